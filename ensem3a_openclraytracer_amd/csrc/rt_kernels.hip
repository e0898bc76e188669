// HIP kernels of the MI355X path tracer (gfx950 / CDNA4).
//
// One work-item per pixel, like the reference kernel (Raytracing.cl:161-221),
// but the per-pixel work is restructured for a 64-wide wavefront:
//
//  * the nested spp x bounce loops of Raytracing.cl:191-209 / naiveGI
//    (Raytracing.cl:46-151) become ONE flat loop whose every iteration traces
//    exactly one ray per lane (bounce ray or sun ray).  A lane whose path ends
//    starts its next sample in the same iteration, so lanes never wait for the
//    longest path of the wave; only the per-ray traversal length diverges.
//    The RNG stream of a pixel is consumed in exactly the reference order, so
//    results are unchanged.
//  * BVH traversal (MathLib.cl:234-288) has two implementations:
//      REF  - the reference's pre-order DFS over its own 9-float AoS nodes,
//             true divisions in the slab test, 20-slot stack with silent drop.
//             Bit-identical to the CPU oracle.
//      FAST - a BVH2 whose nodes carry both child boxes (64 B, four float4
//             loads), reciprocal-direction slab tests, closest-child-first
//             descent, t-culling against the best hit, and a tie break on the
//             leaf's rank in the reference DFS order, so the closest hit is
//             the one the reference selects (first found among equal k).
//    Both keep the per-ray stack in LDS, one column per work-item
//    ([depth][blockDim] ints: lane-consecutive, bank-conflict free).
//
// Numerics: every OpenCL builtin of the reference is taken from rtm.h and the
// file is compiled with -ffp-contract=off (see rtm.h).
#include <mutex>
#include <vector>

#include "rt_device.h"

namespace rt {

namespace {

// A pixel's state between two adds of a progressive accumulation (the ACC instantiations; layout of
// FrameParams::pilot_state): the sum, the cached camera hit, the RNG words and the samples done
__device__ __forceinline__ void save_state(float4* __restrict__ st, int p, rtm_f3 acc, float kc, uint32_t seed0,
                                           uint32_t seed1, int tc, int s) {
    st[2 * (int64_t)p] = make_float4(acc.x, acc.y, acc.z, kc);
    st[2 * (int64_t)p + 1] =
        make_float4(__uint_as_float(seed0), __uint_as_float(seed1), __int_as_float(tc), __int_as_float(s));
}

// One persistent lane = one pixel at a time.  Lanes that finish their pixel
// take the next pixel index from a global counter: the wave ballots the lanes
// that need work, one lane adds the count to the counter, and each lane takes
// base + (its rank among the requesting lanes) -- so no lane idles while the
// rest of its wave finishes a slower pixel.  Per loop iteration every busy
// lane traces exactly one ray (primary, bounce or sun ray).
// ACC: an add of a progressive accumulation (rt_internal.h: F.pilot_state its state, F.pilot the samples done,
// one pass) -- instantiations of their own, so that
// the one-shot kernels keep their code and registers.  kAccAdd: every pixel of the tile, from the uniform base
// F.pilot to F.spp.  kAccListed (rt_accum_add_selected; compiled in rt_adaptive.hip's translation unit only): the
// pixels of a list (F.pilot_order; its length a device word, F.pilot_cost), each from the count s its state
// holds to s + F.spp -- base and limit are per lane (slimit below)
[[maybe_unused]] constexpr int kAccAdd = 1;
constexpr int kAccListed = 2;
// BRUTE_: the brute-force loop (0 none, 1 lock-step, 2 teams, 3 clustered), + kBruteSliced for the launches
// that hand out sample slices (FrameParams::slices; one lane per pixel: 1 and 3 only) -- instantiations of
// their own again, so that an unsliced launch runs the code it ran without them
constexpr int kBruteSliced = 4;
// ... and + kBruteRefill for the launches with a refill threshold (FrameParams::refill > 1; one lane per pixel
// again), so that a launch without one -- the small tiles, where the threshold measured slower -- runs the code
// it ran before.  The instrumented and logging kernels (COUNT, LOG) carry the threshold's code without the flag
constexpr int kBruteRefill = 8;
// ... and + kBruteLean (rt_internal.h: 16) for the one-shot launches brute_lean_frame admits -- every material emissive
// or diffuse, no IBL term, one pass, fixed_point and sun_cache on -- whose loop holds none of the glossy, glass, IBL
// and pilot code and reads no flag that the rule has fixed.  Every operation that shapes a bit stays: the frame is
// the general kernel's
// ... and + kBrutePrimary (32) / kBrutePrepass (64; rt_internal.h) for the lean sliced launches whose camera rays a
// pre-pass traces: kBrutePrepass | loop is that pre-pass -- this kernel's staging prologue, so the trace reads the
// records the loop kernel's trace reads, then one camera ray per tile pixel, its hit written as the pixel's slice
// record -- and + kBrutePrimary the loop that starts every job from such a record
template <int TRAV, bool COUNT, bool LOG = false, bool SMEM = false, bool OVF = false, int BRUTE_ = 0, int ACC = 0>
// amdgpu_waves_per_eu(5): the register allocator keeps the kernel at 96 VGPRs, i.e. 5 waves per SIMD
// (one register more costs a wave per SIMD and ~10 % on C2); the product instantiations fit without
// spills, the instrumented (COUNT) ones spill a few registers to scratch.
#ifndef RT_RENDER_WAVES
#define RT_RENDER_WAVES 5   // variant builds: another waves-per-SIMD target for render_kernel
#endif
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_RENDER_WAVES))) render_kernel(DevScene S, FrameParams F, float* __restrict__ out,
                                               unsigned long long* __restrict__ counts,
                                               unsigned int* __restrict__ work_counter,
                                               const LaunchConst* __restrict__ lconst) {
    constexpr int BRUTE = BRUTE_ & 3;
    constexpr bool SLICED = (BRUTE_ & kBruteSliced) != 0;
    static_assert(!SLICED || BRUTE == 1 || BRUTE == 3, "sample slices: the one-lane brute-force loops");
    constexpr bool kRefill = (BRUTE == 1 || BRUTE == 3) && ((BRUTE_ & kBruteRefill) != 0 || COUNT || LOG);
    static_assert(!(BRUTE_ & kBruteRefill) || BRUTE == 1 || BRUTE == 3, "refill threshold: the one-lane brute-force loops");
    constexpr bool LEAN = (BRUTE_ & kBruteLean) != 0;
    static_assert(!LEAN || ((BRUTE == 1 || BRUTE == 3) && TRAV == TRAV_FAST && !COUNT && !LOG && !ACC && RT_SHADE_ROWS),
                  "lean: the one-lane one-shot product kernels");
    constexpr bool PRE = (BRUTE_ & kBrutePrimary) != 0;       // every job starts from its pixel's record
    constexpr bool PREPASS = (BRUTE_ & kBrutePrepass) != 0;   // the kernel that writes those records
    static_assert(!PRE || (LEAN && SLICED), "camera rays in a pre-pass: the lean sliced kernels");
    static_assert(!PREPASS || (BRUTE_ == (kBrutePrepass | 1) || BRUTE_ == (kBrutePrepass | 3)), "the pre-pass: one per loop");
    static_assert(!PREPASS || (TRAV == TRAV_FAST && !COUNT && !LOG && !SMEM && !OVF && !ACC && RT_SHADE_ROWS), "the pre-pass: a product kernel");
    extern __shared__ __attribute__((aligned(16))) int lds_stack[];
    const int B = blockDim.x;
    int* stk = lds_stack + threadIdx.x;
    const LaneStack lst = lane_stack(S, lds_stack);
    Cnt c{};
    // BRUTE (small scenes, brute-force traversal): the MT batches' triangle records and all shading
    // tables (hit records, hemisphere frames, materials) are staged in LDS behind the per-wave regions
    const float4* mtrec = nullptr;
    const float4* boxrec = nullptr;
    const float4* tshade = S.tri_shade;
    const float4* tframe = S.tri_frame;
    const float* tmat = S.mat;
    // ROWS (the one-lane brute-force kernels): in place of tri_shade's copy and the material table's, one row of two
    // float4 per triangle, n.xyz type | colour.xyz rough -- copies of the words tri_shade and the triangle's material
    // hold, so a shading look-up is one read and not a read of the material's index with a dependent read of the
    // table.  The layout, which brute_lds_bytes (rt_device.h) prices: records | the team kernel's boxes | rows, or
    // tri_shade and behind the frames the materials | frames | the clustered loop's slots and the shell's rows
    constexpr bool ROWS = RT_SHADE_ROWS && (BRUTE == 1 || BRUTE == 3);   // (RT_SHADE_ROWS=0: an A/B build without them)
    const float4* trow = nullptr;
    if (BRUTE) {
        float4* lr = reinterpret_cast<float4*>(reinterpret_cast<char*>(lds_stack) + (B / 64) * BRUTE_WAVE_LDS);
        float4* ls = lr + 3 * S.nbrute;
        if (BRUTE == 2) {   // the distinct leaf boxes (team box tests)
            for (int q = threadIdx.x; q < 2 * S.nbox; q += B) ls[q] = S.brute_box[q];
            boxrec = ls;
            ls += 2 * S.nbox;
        }
        float4* lf = ls + (ROWS ? 2 : 1) * S.ntri;
        float* lm = reinterpret_cast<float*>(lf + 3 * S.ntri);
        stage_mt_records(lr, S.brute, S.nbrute);   // (rt_device.h: the batches' own layout)
        for (int q = threadIdx.x; q < 3 * S.ntri; q += B) lf[q] = S.tri_frame[q];
        if constexpr (ROWS) {
            for (int q = threadIdx.x; q < S.ntri; q += B) {
                const float4 sh = S.tri_shade[q];
                const float* m = S.mat + kMatF * __float_as_int(sh.w);
                ls[2 * q] = make_float4(sh.x, sh.y, sh.z, m[0]);
                ls[2 * q + 1] = make_float4(m[1], m[2], m[3], m[4]);
            }
            trow = ls;
        } else {
            for (int q = threadIdx.x; q < S.ntri; q += B) ls[q] = S.tri_shade[q];
            for (int q = threadIdx.x; q < kMatF * S.nmat; q += B) lm[q] = S.mat[q];
            tshade = ls;
            tmat = lm;
        }
        if (BRUTE == 3) {   // the clustered loop's item tests read their slots here
            float4* lc = reinterpret_cast<float4*>(lm + (ROWS ? 0 : kMatF * S.nmat));   // (behind the table, where it is staged)
            for (int q = threadIdx.x; q < 2 * S.ncslot; q += B) lc[q] = S.brute_cbox[q];
            // ... and the shell's rows behind them (rt_layout.h kShellRows; trace_brute_compact's one queue step
            // reads a lane's face's row), at boxrec + S.shell
            if (S.shell)
                for (int q = threadIdx.x; q < 2 * kShellRows; q += B) lc[S.shell + q] = S.brute_cbox[S.shell + kShellRowF4 + q];
            boxrec = lc;
        }
        __syncthreads();
        mtrec = lr;
        tframe = lf;
    }
    // (RT_CHAIN_STAMPS, rt_device.h: the clustered product kernel's section clocks, in its wave's LDS area)
    // -- every instantiation whose trace stamps (trace_brute_compact<COUNT, CLU>: CLU && !COUNT) zeroes and flushes them
    constexpr bool STAMPS = RT_CHAIN_STAMPS && BRUTE == 3 && !COUNT;
    [[maybe_unused]] char* const stamp_wl = reinterpret_cast<char*>(lds_stack) + (threadIdx.x >> 6) * BRUTE_WAVE_LDS;
    if constexpr (STAMPS) {
        if ((threadIdx.x & 63) == 0) {
            unsigned long long* st = reinterpret_cast<unsigned long long*>(stamp_wl + BRUTE_STAMP_OFF);
            for (int q = 0; q < kStampN; ++q) st[q] = 0;
            st[kStampN] = clock64();
        }
    }
    const LaunchConst& C = *lconst;   // uniform: scalar loads, no VGPRs
    // SMEM: the whole BVH2 node array and triangle array of a small scene are
    // staged in LDS behind the stacks, once per (persistent) block.
    const float4* nodes = S.nodes;
    const float4* tris = S.tri_fast;
    if (SMEM) {
        float4* ln = reinterpret_cast<float4*>(lds_stack + 2 * S.stack_lds * B);
        float4* lt = ln + kNodeF4 * S.nnodes;
        for (int q = threadIdx.x; q < kNodeF4 * S.nnodes; q += B)
            ln[(q % kNodeF4) * S.nnodes + q / kNodeF4] = S.nodes[q];
        for (int q = threadIdx.x; q < 3 * S.ntri; q += B) lt[q] = S.tri_fast[q];
        __syncthreads();
        nodes = ln;
        tris = lt;
    }
    const int W = F.width;
    const int imgSize = (int)F.npix;
    const float e3 = F.env[3], e4 = F.env[4];
    const int spp = F.spp, maxB = F.max_bounce;
    // (a listed add hands out the list's entries: its length is read once, and made wave-uniform for the hand-out)
    const unsigned int nloc = ACC == kAccListed ? (unsigned int)__builtin_amdgcn_readfirstlane((int)*F.pilot_cost)
                                                : (unsigned int)F.nloc;
    const int lane = threadIdx.x & 63;
    const int ts = BRUTE == 2 ? F.team : 1;                      // lanes per pixel (1, 2, 4, 8)
    const int team_lane0 = lane & ~(ts - 1);
    const bool team_leader = lane == team_lane0;
    const unsigned long long team_leaders = ts == 1 ? ~0ull : ts == 2 ? 0x5555555555555555ull
                                             : ts == 4 ? 0x1111111111111111ull : 0x0101010101010101ull;

    // The pre-pass of a lean sliced launch (kBrutePrepass; launch_pick runs it between make_const_kernel and the loop
    // kernel): for tile pixel p what the loop's hand-out and PRIMARY trip do for a new pixel -- the frame pixel i, its
    // camera ray, that ray's trace over the records staged above (the loop kernel's layout and the loop's trace: the
    // same bits) -- written as the pixel's slice record in slice_publish's layout: no sample done, no shadow ray
    // cached.  A padding pixel (i >= npix: a partial last row) gets "all done", what its slice 0 publishes in the
    // other sliced kernels.  Plain stores: the kernel boundary orders them before the loop kernel's loads, and every
    // launch writes every record and every samples-done word of its tile (no memset, nothing kept from a frame)
    if constexpr (PREPASS) {
        for (int64_t p0 = (int64_t)blockIdx.x * B; p0 < F.nloc; p0 += (int64_t)gridDim.x * B) {
            const int64_t pp = p0 + threadIdx.x;
            if (pp >= F.nloc) continue;
            const int krow = (int)pp / W;
            const int col = (int)pp - krow * W;
            const int64_t i64 = ((int64_t)F.row0 + (int64_t)krow * F.row_step) * W + col;
            float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 1000.0f), r2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            uint32_t i0 = 0, w0 = 0, s0 = (uint32_t)spp;
            if (i64 < F.npix) {
                const rtm_f3 d = camera_dir(C, W, (int)i64);
                const Hit h = trace<TRAV, COUNT, SMEM, OVF, true, BRUTE == 3>(S, nodes, tris, C.position, d, stk, B, lst, c, mtrec, ts, boxrec);
                r0.w = h.k;
                r2 = make_float4(d.x, d.y, d.z, 0.0f);
                i0 = (uint32_t)i64;
                w0 = (uint32_t)(h.tri + 1);   // (| (sun0 + 2) << 16 with sun0 = -2)
                s0 = 0u;
            }
            float4* st = F.slice_state + 3 * pp;
            st[0] = r0;                                                                             // acc.xyz | kc
            st[1] = make_float4(__uint_as_float(i0), 0.0f, __uint_as_float(w0), __uint_as_float(s0));   // seed0 seed1 | w s
            st[2] = r2;                                                                             // cd
            F.slice_ready[pp] = s0;
        }
    }

    int phase = FETCH;
    PixelQueue pq;
    pq.per = (F.handout && (LEAN || F.pass != 2)) ? (unsigned)(((ACC == kAccListed ? (int64_t)nloc : F.nloc) + kGroups - 1) / kGroups) : 0u;   // pass 2: cost order, interleaved
    // FrameParams::refill = R rides in the hand-out's word, which the loop keeps anyway (a scalar register of
    // its own spills others that the shading reads)
    if constexpr (kRefill) pq.dry = F.refill > 1 ? (unsigned)min(F.refill, 64) << kQueueRefillShift : 0u;
    int p = 0, i = 0;
    bool logme = false;
    uint32_t seed0 = 0, seed1 = 0;
    rtm_f3 cd = rtm_v3(0, 0, 0);              // camera ray direction (origin = C.position)
    float kc = 1000.0f;                       // cached primary hit
    int tc = -1;
    // the ray being shaded is not kept: at bounce 0 it is the camera ray (C.position, cd, hit kc),
    // later the bounce ray just traced (Bo, Bd, hit k) -- fewer registers live across the trace
    rtm_f3 so = rtm_v3(1, 1, 1);
    float k = 1000.0f;
    int tri = -1, j = 0;
    rtm_f3 Bo = rtm_v3(0, 0, 0), Bd = rtm_v3(0, 0, 0);
    rtm_f3 acc = rtm_v3(0, 0, 0);
    int s = 0;
    // the sample count the pixel stops at: F.spp, or in a listed add the pixel's own (the s it restored + F.spp).
    // (A named lambda with the choice in an if constexpr: of the forms tried, the one that leaves the other
    // instantiations' code as it was)
    [[maybe_unused]] int plim = 0;
    auto slimit = [&]() __attribute__((always_inline)) { if constexpr (ACC == kAccListed) return plim; else return spp; };
    int cost = 0;   // pass 1: rays this pixel traced (pilot_cost)
    int sun0 = -2;  // the first bounce's shadow-ray hit (-1 = miss; -2 = not traced yet)
    unsigned long long t_prev = 0;   // COUNT: the wave clock at the previous loop head
    // COUNT, lane 0 for its wave: loop iterations that ran the hand-out block (take_pixel / take_job and the job's
    // start-up) and the lanes that asked for a job in them -- counts[15] and [16], after the counters of Cnt
    [[maybe_unused]] unsigned long long refill_ev = 0, refill_lanes = 0;
    // pass 1 (FrameParams::pass): after the pilot samples, save the pixel's state for pass 2; the
    // pixel is written (and its cost set to 0) when all its samples are done
    auto save_pilot = [&]() __attribute__((always_inline)) {
        F.pilot_state[2 * (int64_t)p] = make_float4(acc.x, acc.y, acc.z, kc);
        F.pilot_state[2 * (int64_t)p + 1] =
            make_float4(__uint_as_float(seed0), __uint_as_float(seed1), __int_as_float(tc), __int_as_float(s));
        F.pilot_cost[p] = s >= spp ? 0u : (unsigned)cost;
    };

    // sample slices (SLICED; one-pass launches): as in render_resume_kernel, lim is the sample count this
    // job stops at and, while the job waits for the slice before it (WAIT_SLICE), the job's slice index (s is
    // then the sample count that slice ends at: the poll's operand).
    // F.slices = K | tail << 8: only the last tail / 256 of the pixels are sliced, the rest are whole jobs handed
    // out before them (take_pixel), so the hand-offs are paid where the frame ends and nowhere else.
    // The hand-off carries sun0 beside tc (16 bits each: the scene is staged in LDS, ntri + 2 < 2^16,
    // launch_pick), so a pixel traces its first bounce's shadow ray once, not once per slice, and the camera
    // ray's direction: a job that continues a pixel divides nothing and runs no camera_dir (with a job
    // ending in nearly every round of a wave, that start-up is run by the whole wave every round)
    const unsigned nsl = SLICED ? (unsigned)F.slices & 0xffu : 1u;
    const unsigned stail = SLICED ? (unsigned)F.slices >> 8 : 0u;
    const int sb = ACC ? F.pilot : 0;   // (ACC: the samples of earlier adds, rt_internal.h)
    // slice_end (rt_device.h) without its division: (k + 1) n / K = (k + 1) (n / K) + (k + 1) (n % K) / K, the
    // last quotient of a number below 16 x 15 by K <= 16 through a 16-bit reciprocal (exact below 2^16 / 15)
    const unsigned sl_q = (unsigned)(spp - sb) / nsl, sl_r = (unsigned)(spp - sb) % nsl, sl_m = (65536u + nsl - 1u) / nsl;
    auto send = [&](unsigned k) { return sb + (int)((k + 1u) * sl_q + (((k + 1u) * sl_r * sl_m) >> 16)); };
    int lim = spp;
    auto save_slice = [&](rtm_f3 cdv) __attribute__((always_inline)) {
        slice_publish(F, (gu64*)(F.slice_state + 3 * (int64_t)p), p, acc, kc, seed0, seed1,
                      (unsigned)(tc + 1) | ((unsigned)(sun0 + 2) << 16), s, true, cdv);
    };

    while (!PREPASS) {   // (the pre-pass has run its own loop, above: it goes on to the stamps' flush)
        if constexpr (STAMPS) chain_stamp(stamp_wl, kStampRest);
        // instrumented build: wave cycles in the trace (cyc_trav) and in the rest of the loop (cyc_shade:
        // every iteration's time, the trace's subtracted below; unsigned wrap-around cancels)
        if (COUNT && lane == 0) {
            const unsigned long long now = clock64();
            if (t_prev) c.cyc_shade += now - t_prev;
            t_prev = now;
        }
        // -- refill: ballot the lanes that need a pixel, one atomic per wave --
        // teams (BRUTE, F.team lanes per pixel): one bit per team, the team's lanes take the same pixel
        unsigned long long need = __ballot(phase == FETCH) & team_leaders;
        // the one-lane brute-force loops (FrameParams::refill = R > 1): the block below is stepped through by
        // the whole wave for however few lanes ask, so the free lanes wait until R of them ask together.  They
        // never wait (a) with R lanes free, (b) in a wave none of whose lanes holds a ray or a sample to shade --
        // need is cleared only while such a lane exists, and every such lane ends its job after finitely many
        // rounds, so a waiting lane is always served -- or (c) once the hand-out is near its end (take_pixel
        // NEAR clears R).  A finished job is published where it ends (store_pixel, save_slice: below), never
        // behind a waiting lane
        if constexpr (kRefill) {
            if (need && (unsigned)__popcll(need) < (pq.dry >> kQueueRefillShift)) {
                const unsigned long long busy = __ballot(phase != FETCH && phase != DONE && phase != WAIT_SLICE);
                if (busy) need = 0;
            }
        }
        if (COUNT && need && lane == 0) {
            refill_ev++;
            refill_lanes += (unsigned)__popcll(need);
        }
        // PRE: a job whose record the pre-pass wrote (a whole pixel, or slice 0) -- complete before the launch, so it
        // is read below without a poll
        [[maybe_unused]] bool first = false;
        if (need) {
            unsigned sl = kWholeJob;   // SLICED: the job's slice, or a whole pixel
            unsigned int q;
            if constexpr (SLICED) q = take_job<kRefill>(pq, need, team_lane0, work_counter, nloc, lane, nsl, stail, sl);
            else q = take_pixel<kRefill>(pq, need, team_lane0, work_counter, nloc, lane);
            if constexpr (PRE) {
                // every job starts from its pixel's record (below), which holds all that depends on the pixel's
                // number: lim is the slice whose end the job stops at -- the last one for a whole job, send(K - 1) =
                // spp -- and s the count that a job of slice k > 0 waits for.  A padding pixel's record says "all done"
                if (phase == FETCH) {
                    if (q < nloc) {
                        p = (int)q;
                        first = sl == kWholeJob || sl == 0;
                        lim = sl == kWholeJob ? (int)nsl - 1 : (int)sl;
                        s = send(sl - 1u);   // (unused by a first job)
                        phase = WAIT_SLICE;
                    } else {
                        phase = DONE;
                    }
                }
            } else
            if (SLICED && phase == FETCH && q < nloc && sl != kWholeJob && sl > 0) {
                // continues a pixel once its slice sl - 1 is done (below): all it needs is in that slice's state
                p = (int)q;
                lim = (int)sl;
                s = send(sl - 1u);
                phase = WAIT_SLICE;
            } else if (phase == FETCH) {
                const bool whole = !SLICED || sl == kWholeJob;
                bool ok = q < nloc;
                if (ok) {
                    if constexpr (LEAN) p = (int)q;   // (one pass: no cost order)
                    else p = (ACC == kAccListed || F.pass == 2) ? (int)F.pilot_order[q] : (int)q;
                    const int krow = p / W;
                    const int col = p - krow * W;
                    const int64_t i64 = ((int64_t)F.row0 + (int64_t)krow * F.row_step) * W + col;
                    ok = i64 < F.npix;
                    i = (int)i64;
                }
                if (ok) {
                    if constexpr (SLICED) {   // i < npix = imgSize (ok above; npix < 2^31, launch_pick): no division
                        seed0 = (uint32_t)i;
                        seed1 = 0;
                    } else {
                        seed0 = (uint32_t)(i % imgSize);
                        seed1 = (uint32_t)(i / imgSize);
                    }
                    cd = camera_dir(C, W, i);
                    acc = rtm_v3(0, 0, 0);
                    s = 0;
                    cost = 0;
                    sun0 = -2;
                    phase = PRIMARY;
                    logme = LOG && i == F.log_pixel;
                    if (!LEAN && F.pass == 2) {   // continue from the pilot state: camera hit cached, sample s next
                        const float4 a = F.pilot_state[2 * (int64_t)p], b = F.pilot_state[2 * (int64_t)p + 1];
                        acc = rtm_v3(a.x, a.y, a.z);
                        kc = a.w;
                        seed0 = __float_as_uint(b.x);
                        seed1 = __float_as_uint(b.y);
                        tc = __float_as_int(b.z);
                        s = __float_as_int(b.w);
                        tri = tc; j = 0;
                        so = rtm_v3(1, 1, 1);
                        phase = s >= spp ? FETCH : PREP;   // finished in pass 1: already written
                    }
                    if constexpr (ACC) if (ACC == kAccListed || F.pilot > 0) {   // continue the accumulation: camera hit cached, sample s next
                        const float4 a = F.pilot_state[2 * (int64_t)p], b = F.pilot_state[2 * (int64_t)p + 1];
                        acc = rtm_v3(a.x, a.y, a.z);
                        kc = a.w;
                        seed0 = __float_as_uint(b.x);
                        seed1 = __float_as_uint(b.y);
                        tc = __float_as_int(b.z);
                        s = __float_as_int(b.w);
                        tri = tc; j = 0;
                        so = rtm_v3(1, 1, 1);
                        phase = PREP;
                        if constexpr (ACC == kAccListed) plim = s + spp;
                    }
                    if constexpr (SLICED) lim = whole ? spp : send(0);
                } else {
                    // past the tile, or a padding pixel of a partial last row (its hand-out group, pass 2's
                    // cost order, or later sample slices may still hold real pixels): the lane retires once the queue is dry
                    // (SLICED: slice 0 of a padding pixel says "all done" to the jobs of its later slices, which
                    // do not look at the pixel's number)
                    if constexpr (SLICED) { if (q < nloc && !whole) { s = spp; save_slice(cd); } }
                    phase = q < nloc ? FETCH : DONE;
                }
            }
        }
        if constexpr (SLICED) {
            // the previous slice's samples done, published by the lane that ran it (save_slice): once the
            // count is there the job continues from that lane's state, in this same iteration
            bool take = false;
            if constexpr (PRE) take = phase == WAIT_SLICE && (first || slice_ready(F, p, (unsigned)s));
            else take = phase == WAIT_SLICE && slice_ready(F, p, (unsigned)s);
            if (take) {
                unsigned w;
                gu64* st = (gu64*)(F.slice_state + 3 * (int64_t)p);
                slice_take(st, acc, kc, seed0, seed1, w, s);
                cd = slice_take_cd(st);
                tc = (int)(w & 0xffffu) - 1;
                sun0 = (int)(w >> 16) - 2;
                tri = tc; j = 0;
                so = rtm_v3(1, 1, 1);
                lim = send((unsigned)lim);
                phase = s >= spp ? FETCH : PREP;   // finished early (a sample that draws nothing): written
            }
        }
        if (__all(phase == DONE)) break;
        if (SLICED && __all(phase == DONE || phase == WAIT_SLICE)) __builtin_amdgcn_s_sleep(8);
        if (COUNT && lane == 0) c.wave_outer++;
        if (phase == DONE || phase == FETCH || (SLICED && phase == WAIT_SLICE)) continue;   // FETCH: a pass-2 pixel finished in pass 1

        if (phase == PREP) {
            // naiveGI loop head for bounce j (Raytracing.cl:46-79); may complete samples without tracing
            bool done = true;
            const bool cam = j == 0;
            const rtm_f3 Ro = cam ? C.position : Bo, Rd = cam ? cd : Bd;
            const float kh = cam ? kc : k;
            if constexpr (LEAN) {
                // max_bounce >= 0: j never passes it (the bounce at j == maxB ends the sample, below).  e4 is +0: the
                // IBL term of a ray that left the scene is so x 0 -- (so x 0) x +0 keeps its bits, NaN and sign.  A
                // surface is emissive (type 0) or diffuse: its row says which, and no other type's code is here
                if (tri < 0) {
                    so = rtm_mul(so, rtm_v3(0.0f, 0.0f, 0.0f));
                } else {
                    const float4 sh = trow[2 * tri], r1 = trow[2 * tri + 1];
                    if ((int)sh.w == 0) {
                        so = rtm_scale(so, r1.w);
                    } else {
                        const float4 f2 = tframe[3 * tri + 2];
                        const rtm_f3 nn = xyz(f2);
                        float invPdf = 0.0f;
                        Bd = hemi_cosine(xyz(sh), tframe[3 * tri], tframe[3 * tri + 1], f2, &seed1, &seed0, &invPdf);
                        const rtm_f3 brdf = rtm_scale(rtm_v3(r1.x, r1.y, r1.z), 1.0f / 3.14f);
                        const rtm_f3 nd = dev_normalize(Rd);
                        Bo = rtm_v3(fmaf(nd.x, kh, Ro.x), fmaf(nd.y, kh, Ro.y), fmaf(nd.z, kh, Ro.z));
                        const float att = invPdf * rtm_fabs(rtm_dot(Bd, nn));
                        so = rtm_scale(rtm_mul(so, brdf), att);
                        phase = BOUNCE;
                        done = false;
                    }
                }
            } else if (j > maxB) {
                // naiveGI's loop never entered (maxBounce < 0): the sample stays 1
            } else if (tri < 0) {
                so = rtm_scale(rtm_mul(so, sample_ibl_if<COUNT>(S, C, Rd, e4, c)), e4);
            } else {
                const float4 sh = ROWS ? trow[2 * tri] : tshade[tri];
                const rtm_f3 n = xyz(sh);
                const Mat cm = ROWS ? row_mat(sh, trow[2 * tri + 1]) : load_mat(tmat, __float_as_int(sh.w));
                if (cm.type == 0) {
                    so = rtm_scale(so, cm.rough);
                } else {
                    const float4 f2 = tframe[3 * tri + 2];
                    const rtm_f3 nn = xyz(f2);
                    float invPdf = 0.0f;
                    rtm_f3 brdf = rtm_v3(0, 0, 0);
                    if (COUNT) count_event(c, cm.type);
                    if (cm.type == 1) {
                        Bd = hemi_cosine(n, tframe[3 * tri], tframe[3 * tri + 1], f2, &seed1, &seed0,
                                         &invPdf);
                        brdf = rtm_scale(cm.color, 1.0f / 3.14f);
                    } else if (cm.type == 2) {
                        Bd = hemi_uniform(n, tframe[3 * tri], tframe[3 * tri + 1], f2, &seed1, &seed0,
                                          &invPdf);
                        brdf = brdf_ggx(cm.color, cm.rough, rtm_scale(Rd, -1.0f), Bd, n);
                    } else {
                        Bd = Rd;
                        brdf = cm.color;
                        invPdf = 1.0f / rtm_fabs(rtm_dot(Bd, nn));
                    }
                    const rtm_f3 nd = dev_normalize(Rd);
                    Bo = rtm_v3(fmaf(nd.x, kh, Ro.x), fmaf(nd.y, kh, Ro.y), fmaf(nd.z, kh, Ro.z));
                    // attenuation depends only on pre-trace values (Raytracing.cl:86-87): apply now
                    const float att = invPdf * rtm_fabs(rtm_dot(Bd, nn));
                    so = rtm_scale(rtm_mul(so, brdf), att);
                    phase = BOUNCE;
                    done = false;
                }
            }
            if (done) {
                if (LOG && logme) log_event(F, 3.0f, s + 1, rtm_v3(0, 0, 0), rtm_v3(0, 0, 0), 0.0f, 0, so);
                acc = rtm_add(acc, so);
                if (COUNT) c.samples++;
                ++s;
                // A sample that ends at its first loop head (j == 0: no bounce sampled) drew no random
                // numbers, so the RNG state is unchanged and every later sample of the pixel is this
                // sample again (same cached camera hit, same state): their colours are added in order,
                // bit for bit the reference's sum (FrameParams::fixed_point).
                if (TRAV == TRAV_FAST && (LEAN || F.fixed_point) && j == 0 && !(LOG && logme)) {
                    if (COUNT) c.samples += (unsigned long long)max(slimit() - s, 0);
                    for (; s < slimit(); ++s) acc = rtm_add(acc, so);
                }
                if (s >= slimit()) {
                    phase = FETCH;
                    if (team_leader) store_pixel(out, p, acc, slimit());
                    if (!LEAN && F.pass == 1) save_pilot();
                    if constexpr (ACC) { if (team_leader) save_state(F.pilot_state, p, acc, kc, seed0, seed1, tc, s); }
                    if constexpr (SLICED) { if (lim < spp) save_slice(cd); }   // done early: its later slices find nothing to do
                } else if (!LEAN && F.pass == 1 && s >= F.pilot) {
                    save_pilot();
                    phase = FETCH;
                } else if (SLICED && s >= lim) {
                    save_slice(cd);
                    phase = FETCH;
                } else {
                    tri = tc; j = 0;
                    so = rtm_v3(1, 1, 1);
                }
                continue;
            }
        }

        // -- one ray per busy lane --
        // (PRE: no lane is ever in PRIMARY -- the pre-pass traced the camera rays)
        const rtm_f3 to = (!PRE && phase == PRIMARY) ? C.position : Bo;
        const rtm_f3 td = (!PRE && phase == PRIMARY) ? cd : ((phase == BOUNCE) ? Bd : C.sun);
        const unsigned long long t_tr = COUNT ? clock64() : 0;
        if constexpr (STAMPS) chain_stamp(stamp_wl, kStampHead);
        const Hit h = trace<TRAV, COUNT, SMEM, OVF, BRUTE != 0, BRUTE == 3>(S, nodes, tris, to, td, stk, B, lst, c, mtrec, ts, boxrec);
        if (COUNT && lane == __ffsll((long long)__ballot(1)) - 1) {   // the first tracing lane, once per wave
            const unsigned long long dt = clock64() - t_tr;
            c.cyc_trav += dt;
            c.cyc_shade -= dt;
        }
        ++cost;
        bool finish = false;
        if (!PRE && phase == PRIMARY) {
            tc = h.tri;
            kc = h.k;
            tri = tc; j = 0;
            so = rtm_v3(1, 1, 1);
            phase = PREP;
            if (!LEAN && spp <= 0) {   // reference: output = 0/0 -> NaN -> clamp gives 1
                if (team_leader) store_pixel(out, p, acc, spp);
                phase = FETCH;
            }
            continue;
        }
        if (LOG && logme) {
            const int hm = h.tri >= 0 ? __float_as_int(S.tri_shade[h.tri].w) : 0;   // (the global table: the rows hold no index)
            log_event(F, phase == BOUNCE ? 1.0f : 2.0f, j, Bo, td, h.tri >= 0 ? h.k : -1.0f, hm, so);
        }
        int sun_hit = -2;   // the shadow ray's hit for the sun term below (-1 = miss; -2 = no sun term now)
        // the first bounce leaves from the cached camera hit in every sample of the pixel, so its shadow
        // ray towards the sun is the same ray each time: traced once per pixel (FrameParams::fixed_point)
        const bool sun_first = TRAV == TRAV_FAST && (LEAN || F.sun_cache) && j == 0 && !(LOG && logme);
        if (phase == BOUNCE) {
            if (h.tri >= 0) {
                tri = h.tri; k = h.k;
                // (LEAN: the row's type word alone, and the emitter's power word where the type says emitter)
                const Mat bm = LEAN ? Mat{(int)trow[2 * h.tri].w, rtm_v3(0, 0, 0), 0.0f}
                               : ROWS ? row_mat(trow[2 * h.tri], trow[2 * h.tri + 1])
                                      : load_mat(tmat, __float_as_int(tshade[h.tri].w));
                if (bm.type != 0) {
                    if (j == maxB) {
                        so = rtm_v3(0, 0, 0);
                        finish = true;
                    } else {
                        ++j;
                        phase = PREP;
                    }
                } else {
                    so = rtm_scale(so, LEAN ? trow[2 * h.tri + 1].w : bm.rough);
                    finish = true;
                }
            } else if (TRAV == TRAV_FAST && F.sun_skip) {
                sun_hit = -1;   // unlit sun: the shadow ray cannot change the sample (FrameParams::sun_skip)
            } else if (sun_first && sun0 != -2) {
                sun_hit = sun0;   // the first bounce's shadow ray, traced in an earlier sample of the pixel
            } else {
                phase = SUN;
            }
        } else {
            sun_hit = h.tri;
            if (sun_first) sun0 = h.tri;
        }
        if (sun_hit != -2) {  // SUN (Raytracing.cl:115-137)
            if (COUNT) c.sun++;
            if constexpr (LEAN) {
                // neither the surface the bounce left nor an occluder is glass: the sun's light or none, and no row
                // is read.  The IBL term is 0 x e4 = +0; its add stays, since e3 may be -0
                const float l = (sun_hit < 0 ? e3 : 0.0f) + 0.0f;
                so = rtm_mul(so, rtm_v3(l, l, l));
            } else {
                rtm_f3 sunLight = rtm_v3(0, 0, 0);
                const Mat cm = ROWS ? row_mat(trow[2 * tri], trow[2 * tri + 1])
                                    : load_mat(tmat, __float_as_int(tshade[tri].w));
                if (sun_hit < 0 && cm.type != 3) sunLight = rtm_v3(e3, e3, e3);
                if (sun_hit >= 0) {
                    const Mat sm = ROWS ? row_mat(trow[2 * sun_hit], trow[2 * sun_hit + 1])
                                        : load_mat(tmat, __float_as_int(tshade[sun_hit].w));
                    if (sm.type == 3) sunLight = rtm_scale(sm.color, e3);
                }
                const rtm_f3 envLight = rtm_scale(sample_ibl_if<COUNT>(S, C, Bd, e4, c), e4);
                so = rtm_mul(so, rtm_add(sunLight, envLight));
            }
            finish = true;
        }
        if (finish) {
            if (LOG && logme) log_event(F, 3.0f, s + 1, rtm_v3(0, 0, 0), rtm_v3(0, 0, 0), 0.0f, 0, so);
            acc = rtm_add(acc, so);
            if (COUNT) c.samples++;
            ++s;
            if (s >= slimit()) {
                if (team_leader) store_pixel(out, p, acc, slimit());
                if (!LEAN && F.pass == 1) save_pilot();
                if constexpr (ACC) { if (team_leader) save_state(F.pilot_state, p, acc, kc, seed0, seed1, tc, s); }
                phase = FETCH;   // (SLICED: s goes up by one here, so this is the pixel's last slice: lim == spp)
            } else if (!LEAN && F.pass == 1 && s >= F.pilot) {
                save_pilot();
                phase = FETCH;
            } else if (SLICED && s >= lim) {
                save_slice(cd);
                phase = FETCH;
            } else {
                tri = tc; j = 0;
                so = rtm_v3(1, 1, 1);
                phase = PREP;
            }
        }
    }
    if constexpr (STAMPS) {
        if ((threadIdx.x & 63) == 0 && counts) {
            const unsigned long long* st = reinterpret_cast<const unsigned long long*>(stamp_wl + BRUTE_STAMP_OFF);
            for (int q = 0; q < kStampN; ++q) atomicAdd(&counts[q], st[q]);
        }
    }
    if (COUNT) {
        if (!team_leader) {   // a team's lanes repeat its pixel's shading: counted once
            c.env = 0; c.diffuse = 0; c.glossy = 0; c.glass = 0; c.sun = 0; c.samples = 0;
        }
        unsigned long long v[NCOUNTS] = {c.nodes, c.tris, c.rays, c.env, c.dropped, c.wave_trav, c.wave_outer,
                                          c.cyc_shade, c.cyc_trav, c.boxes, c.diffuse, c.glossy, c.glass,
                                          c.sun, c.samples};
#pragma unroll
        for (int q = 0; q < NCOUNTS; ++q) {
            unsigned long long x = v[q];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
            if (lane == 0 && x) atomicAdd(&counts[q], x);
        }
        if (BRUTE && lane == 0) {   // the hand-out's counters: lane 0 keeps its wave's
            atomicAdd(&counts[NCOUNTS], refill_ev);
            atomicAdd(&counts[NCOUNTS + 1], refill_lanes);
        }
    }
}

// FrameParams::step = 0 (auto): one item per step (fast_step) when the node array is at most this
// many bytes (L2-resident scenes, bound by the texture-address unit), descend-until-leaf rounds
// (fast_round) above (C5's 64 MB: bound by the latency of L2 misses; fast_round 1000 vs fast_step
// 944 Msamples/s there)
constexpr size_t kStepMaxBytes = 16u << 20;

// Occupancy: the 4-wide walk (C5) is bound by the latency of dependent L2 misses, so it runs
// kWideWaves waves per SIMD -- the register allocator keeps it at 72 VGPRs with some spilled to
// scratch, and dev_scene keeps kStackLdsWide stack entries per lane in LDS so that the LDS admits
// them.  C5 ms per frame at 4 / 5 / 6 / 7 / 8 waves: 7,214 / 6,432 / 6,045 / 5,890 / 6,040.  The
// BVH2 walk (C3/C4) is bound by the vector memory pipeline and keeps 4 waves with its whole 20-entry
// stack in LDS (5 waves with a 14-entry spilling stack: C3 149 -> 157 ms, C4 475 -> 502 ms).
// (kWideWaves: rt_internal.h)

// TS > 1: teams of TS lanes per pixel walk each ray together (team_step; BVH2 item steps only).
// WIDE: 0 = the BVH2 walk, 1 = the 4-wide walk, 2 = the 4-wide walk with origin-folded dequantisation
// (wide_node DQ; choose_kernel picks it when the camera lies within DevScene::wdq_omax)
template <bool COUNT, bool LOG, bool SMEM, bool OVF, bool STEP, int WIDE, int TS = 1, int ACC = 0>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WIDE ? kWideWaves : 4))) render_resume_kernel(DevScene S, FrameParams F, float* __restrict__ out,
                                                      unsigned long long* __restrict__ counts,
                                                      unsigned int* __restrict__ work_counter,
                                                      const LaunchConst* __restrict__ lconst) {
    extern __shared__ int lds_stack[];
    const int B = blockDim.x;
    // two-pass launches are BVH2-only (the 4-wide walk's pilot measured slower, rt_api.hip setup_pilot):
    // the 4-wide instantiations are one-pass and carry none of the pass code
    const int pass = (WIDE || ACC) ? 0 : F.pass;   // (an accumulation's add is one pass)
    Cnt c{};
    const LaunchConst& C = *lconst;
    const float4* nodes = S.nodes;
    const float4* tris = S.tri_fast;
    if (SMEM) {
        float4* ln = reinterpret_cast<float4*>(lds_stack + 2 * S.stack_lds * B);
        float4* lt = ln + kNodeF4 * S.nnodes;
        for (int q = threadIdx.x; q < kNodeF4 * S.nnodes; q += B)
            ln[(q % kNodeF4) * S.nnodes + q / kNodeF4] = S.nodes[q];
        for (int q = threadIdx.x; q < 3 * S.ntri; q += B) lt[q] = S.tri_fast[q];
        __syncthreads();
        nodes = ln;
        tris = lt;
    }
    const LaneStack lst = lane_stack(S, lds_stack);
    const char* const nb = reinterpret_cast<const char*>(nodes);
    const char* const tb = reinterpret_cast<const char*>(tris);
    const char* const wnb = reinterpret_cast<const char*>(S.wnodes);   // WIDE: 4-wide nodes / leaf records
    const char* const wlb = reinterpret_cast<const char*>(S.wleaves);
    const unsigned kstride = SMEM ? 16u * (unsigned)S.nnodes : 16u;
    const int W = F.width;
    const int imgSize = (int)F.npix;
    const float e3 = F.env[3], e4 = F.env[4];
    const int spp = F.spp, maxB = F.max_bounce;
    // (a listed add hands out the list's entries: its length is read once, and made wave-uniform for the hand-out)
    const unsigned int nloc = ACC == kAccListed ? (unsigned int)__builtin_amdgcn_readfirstlane((int)*F.pilot_cost)
                                                : (unsigned int)F.nloc;
    const int lane = threadIdx.x & 63;
    static_assert(TS == 1 || ((TS == 2 || TS == 4 || TS == 8) && STEP && !WIDE), "team walk: BVH2 item steps");
    const int team_lane0 = lane & ~(TS - 1);
    const bool team_leader = lane == team_lane0;
    const unsigned long long team_leaders = TS == 1 ? ~0ull : TS == 2 ? 0x5555555555555555ull
                                            : TS == 4 ? 0x1111111111111111ull : 0x0101010101010101ull;
    unsigned boff = 0;   // team walk: bottom of this lane's stack (bytes; entries below were stolen)

    int phase = FETCH;
    bool tracing = false;
    PixelQueue pq;
    pq.per = (F.handout && pass != 2) ? (unsigned)(((ACC == kAccListed ? (int64_t)nloc : F.nloc) + kGroups - 1) / kGroups) : 0u;   // pass 2: cost order, interleaved
    FastRay T;
    T.item = 0; T.soff = 0; T.bk = 1000.0f; T.bt = -1; T.brank = -1; T.any = false;
    T.o = rtm_v3(0, 0, 0); T.d = rtm_v3(0, 0, 1); T.ix = T.iy = T.iz = 0.0f;
    int p = 0, i = 0;
    bool logme = false;
    uint32_t seed0 = 0, seed1 = 0;
    rtm_f3 cd = rtm_v3(0, 0, 0);              // camera ray direction (origin = C.position)
    float kc = 1000.0f;                       // cached primary hit (Raytracing.cl:186-187)
    int tc = -1;
    // the ray being shaded is not kept: at bounce 0 it is the camera ray (C.position, cd, hit kc),
    // later the bounce ray just traced (T.o, T.d, hit T.bk) -- fewer registers live across traversal
    rtm_f3 so = rtm_v3(1, 1, 1);
    int tri = -1, j = 0;
    rtm_f3 Bd = rtm_v3(0, 0, 0);   // bounce direction (its origin is T.o while it and the sun ray are traced)
    rtm_f3 acc = rtm_v3(0, 0, 0);
    int s = 0;
    bool drew = false;   // the current sample has drawn random numbers (a diffuse or glossy bounce)
    int cost = 0;        // pass 1: rays this pixel traced (pilot_cost)
    int ndraw = 0;       // pass 1, BVH2 walk: random numbers the pixel drew (its RNG offset, pilot_draws)
    // sample slices (FrameParams::slices): the sample count this job stops at; while the job waits for the
    // slice before it (phase WAIT_SLICE), the job's slice index
    // (one-pass launches, and pass 2 of a pilot launch: the samples after the pilot's sb = F.pilot; slice k
    // of a pixel ends at sb + (k + 1) (spp - sb) / nsl)
    const unsigned nsl = (ACC != kAccListed && TS == 1 && F.slices > 1 && pass != 1) ? (unsigned)F.slices : 1u;   // (a listed add takes none)
    const int sb = (ACC || pass == 2) ? F.pilot : 0;   // (ACC: the samples of earlier adds, rt_internal.h)
    auto sl_end = [&](unsigned k) { return slice_end(sb, spp, nsl, k); };
    int lim = spp;
    // the sample count the pixel stops at: F.spp, or in a listed add the pixel's own (the s it restored + F.spp).
    // (A named lambda with the choice in an if constexpr: of the forms tried, the one that leaves the other
    // instantiations' code as it was)
    [[maybe_unused]] int plim = 0;
    auto slimit = [&]() __attribute__((always_inline)) { if constexpr (ACC == kAccListed) return plim; else return spp; };
    // The deterministic prefix of the pixel's samples (FrameParams::fixed_point; BVH2 walk): a sample's
    // path up to its first diffuse or glossy bounce draws no random number -- it is the cached camera
    // hit followed by straight-through glass bounces (Raytracing.cl:72-77) -- so it is the same path in
    // every sample of the pixel.  The state at the first bounce that draws (bounce j, surface, sample
    // colour so far, and the ray that reached it) is kept once met, and every later sample of the
    // pixel starts there instead of re-tracing the glass chain: the same rays would give the same hits.
    constexpr bool PREFIX = !WIDE;
    bool pre = false;
    int pre_j = 0, pre_tri = -1;
    rtm_f3 pre_so = rtm_v3(1, 1, 1), pre_o = rtm_v3(0, 0, 0), pre_d = rtm_v3(0, 0, 1);
    float pre_k = 1000.0f;
    // The sample's first diffuse or glossy bounce leaves from the same point in every sample (the end of
    // the deterministic prefix), so when its bounce ray escapes, the shadow ray towards the sun
    // (Raytracing.cl:115-124) is the same ray in every sample: its hit is traced once per pixel and kept.
    constexpr bool SUNC = true;
    constexpr int SUN_UNKNOWN = -2;
    int sun_c = SUN_UNKNOWN;   // the first drawing bounce's shadow-ray hit (triangle, -1 for none)
    bool fdb = false;          // the bounce in flight is the sample's first drawing bounce

    auto write_pixel = [&]() __attribute__((always_inline)) {
        if (team_leader) store_pixel(out, p, acc, slimit());
        // ACC: the pixel's last sample of this add: its state for the next add
        if constexpr (ACC) { if (team_leader) save_state(F.pilot_state, p, acc, kc, seed0, seed1, tc, s); }
    };
    // pass 1 (FrameParams::pass): after the pilot samples, save the pixel's state for pass 2; the
    // pixel is written (and its cost set to 0) when all its samples are done
    auto save_pilot = [&]() __attribute__((always_inline)) {
        if (!team_leader) return;
        F.pilot_state[2 * (int64_t)p] = make_float4(acc.x, acc.y, acc.z, kc);
        F.pilot_state[2 * (int64_t)p + 1] =
            make_float4(__uint_as_float(seed0), __uint_as_float(seed1), __int_as_float(tc), __int_as_float(s));
        F.pilot_cost[p] = s >= spp ? 0u : (unsigned)cost;
        if (!WIDE && F.pilot_draws) F.pilot_draws[p] = (uint32_t)ndraw;
    };
    // slices: the pixel's state after this job's slice, for the lane that runs the next one (slice_publish)
    auto save_slice = [&]() __attribute__((always_inline)) {
        if (!team_leader) return;
        slice_publish(F, (gu64*)(F.slice_state + 2 * (int64_t)p), p, acc, kc, seed0, seed1, (unsigned)tc, s);
    };
    auto finish_sample = [&]() __attribute__((always_inline)) {  // output += baseColor; next sample from the cached camera hit
        if (LOG && logme) log_event(F, 3.0f, s + 1, rtm_v3(0, 0, 0), rtm_v3(0, 0, 0), 0.0f, 0, so);
        acc = rtm_add(acc, so);
        if (COUNT) c.samples++;
        ++s;
        if (s >= slimit()) write_pixel();
        const bool stop = (pass == 1 && (s >= slimit() || s >= F.pilot)) || (nsl > 1 && s >= lim);
        if (stop) {
            if (nsl > 1) save_slice();
            else save_pilot();
        }
        // the next sample restarts from the cached camera hit; written as selects so that no branch
        // ends in a store the compiler could merge with the pixel store (that would force the path
        // state into scratch memory through a generic pointer)
        phase = (s >= slimit() || stop) ? FETCH : PREP;
        tri = tc; j = 0;
        so = rtm_v3(1, 1, 1);
        drew = false;
        if (PREFIX && pre) {   // the next sample starts after the deterministic prefix
            tri = pre_tri; j = pre_j;
            so = pre_so;
            T.o = pre_o; T.d = pre_d; T.bk = pre_k;
        }
    };
    // A sample that drew no random numbers (camera ray escaped or on an emitter, or only glass
    // bounces): the RNG state is unchanged, so every later sample of the pixel is this sample again.
    // Their colours are added in order here (finish_sample adds the last), bit for bit the
    // reference's sum (FrameParams::fixed_point).
    auto repeat_fixed = [&]() __attribute__((always_inline)) {
        if (F.fixed_point && !drew && !(LOG && logme)) {
            if (COUNT) c.samples += (unsigned long long)max(slimit() - 1 - s, 0);
            for (; s + 1 < slimit(); ++s) acc = rtm_add(acc, so);
        }
    };
    auto start = [&](rtm_f3 o, rtm_f3 d) __attribute__((always_inline)) {
        ++cost;
        tracing = !fast_init<COUNT>(S, T, o, d, c);
        if (WIDE) T.item = S.wroot_ref;
        if (TS > 1) {   // the team's first lane takes the root; the others steal from it
            if (!team_leader) T.item = NO_ITEM;
            boff = 0;
        }
        T.any = false;
    };

    while (true) {
        const unsigned long long t_iter = COUNT ? clock64() : 0;
        // -- refill: ballot the lanes that need a pixel, one atomic per wave (one pixel per team) --
        const unsigned long long need = __ballot(phase == FETCH) & team_leaders;
        if (need) {
            const unsigned int qj = take_pixel(pq, need, team_lane0, work_counter, nloc, lane, nsl);
            if (phase == FETCH) {
                const unsigned sl = ACC == kAccListed ? 0u : qj / nloc;   // the job's slice (>= nsl: none left; a listed add has none)
                const unsigned q = sl < nsl ? qj - sl * nloc : nloc;
                bool ok = q < nloc;
                if (ok) {
                    p = (ACC == kAccListed || pass == 2) ? (int)F.pilot_order[q] : (int)q;
                    const int krow = p / W;
                    const int col = p - krow * W;
                    const int64_t i64 = ((int64_t)F.row0 + (int64_t)krow * F.row_step) * W + col;
                    ok = i64 < F.npix;
                    i = (int)i64;
                }
                if (ok) {
                    seed0 = (uint32_t)(i % imgSize);
                    seed1 = (uint32_t)(i / imgSize);
                    cd = camera_dir(C, W, i);
                    acc = rtm_v3(0, 0, 0);
                    s = 0;
                    cost = 0;
                    ndraw = 0;
                    pre = false;
                    sun_c = SUN_UNKNOWN;
                    phase = PRIMARY;
                    logme = LOG && i == F.log_pixel;
                    if (sl > 0) {
                        lim = (int)sl;   // continues the pixel once slice sl - 1 is done (below)
                        phase = WAIT_SLICE;
                    } else if (pass == 2) {   // continue from the pilot state: camera hit cached, sample s next
                        const float4 a = F.pilot_state[2 * (int64_t)p], b = F.pilot_state[2 * (int64_t)p + 1];
                        acc = rtm_v3(a.x, a.y, a.z);
                        kc = a.w;
                        seed0 = __float_as_uint(b.x);
                        seed1 = __float_as_uint(b.y);
                        tc = __float_as_int(b.z);
                        s = __float_as_int(b.w);
                        tri = tc; j = 0;
                        so = rtm_v3(1, 1, 1);
                        drew = false;
                        lim = sl_end(0);
                        phase = s >= spp ? FETCH : PREP;   // finished in pass 1: already written
                        if (nsl > 1 && s >= spp) save_slice();   // ... and its later slices have nothing to do
                    } else if (ACC == kAccListed || (ACC && F.pilot > 0)) {   // continue the accumulation: camera hit cached, sample s next
                        const float4 a = F.pilot_state[2 * (int64_t)p], b = F.pilot_state[2 * (int64_t)p + 1];
                        acc = rtm_v3(a.x, a.y, a.z);
                        kc = a.w;
                        seed0 = __float_as_uint(b.x);
                        seed1 = __float_as_uint(b.y);
                        tc = __float_as_int(b.z);
                        s = __float_as_int(b.w);
                        tri = tc; j = 0;
                        so = rtm_v3(1, 1, 1);
                        drew = false;
                        lim = sl_end(0);
                        phase = PREP;
                        if constexpr (ACC == kAccListed) plim = s + spp;
                    } else {
                        lim = sl_end(0);
                        start(C.position, cd);
                    }
                } else {
                    // past the tile, or a padding pixel of a partial last row: with sample slices (jobs handed
                    // out slice-major) or pixels in cost order (pass 2) later jobs of real pixels may still be
                    // queued, so the lane only retires once the queue itself has run dry (q == nloc)
                    phase = q < nloc ? FETCH : DONE;
                }
            }
        }
        if (nsl > 1 && phase == WAIT_SLICE) {
            // slices: the previous slice's samples done, published by the lane that ran it (save_slice); its
            // state is read with sc1 loads (past this CU's L1) once the count is there
            if (slice_ready(F, p, (unsigned)sl_end((unsigned)lim - 1u))) {
                unsigned w;
                slice_take((gu64*)(F.slice_state + 2 * (int64_t)p), acc, kc, seed0, seed1, w, s);
                tc = (int)w;
                tri = tc; j = 0;
                so = rtm_v3(1, 1, 1);
                drew = false;
                lim = sl_end((unsigned)lim);
                phase = s >= spp ? FETCH : PREP;   // finished early (a sample that draws nothing): written
            }
        }
        if (__all(phase == DONE)) break;
        if (nsl > 1 && __all(phase == DONE || phase == WAIT_SLICE)) __builtin_amdgcn_s_sleep(8);
        if (COUNT && lane == 0) c.wave_outer++;

        // -- advance every lane without a ray in flight until it needs one --
        if (!tracing && phase != DONE && phase != FETCH) {
            Hit h{T.bk, WIDE && T.bt >= 0 ? (int)((unsigned)T.bt / 48u) : T.bt};
            if (phase == PRIMARY) {
                tc = h.tri;
                kc = h.k;
                tri = tc; j = 0;
                so = rtm_v3(1, 1, 1);
                drew = false;
                phase = PREP;
                if (spp <= 0) {   // reference: output = 0/0 -> NaN -> clamp gives 1
                    write_pixel();
                    phase = FETCH;
                }
            } else if (phase == BOUNCE) {
                if (LOG && logme) {
                    const int hm = h.tri >= 0 ? __float_as_int(S.tri_shade[h.tri].w) : 0;
                    log_event(F, 1.0f, j, T.o, Bd, h.tri >= 0 ? h.k : -1.0f, hm, so);
                }
                if (h.tri >= 0) {
                    tri = h.tri;
                    const Mat bm = load_mat(S.mat, __float_as_int(S.tri_shade[h.tri].w));
                    if (bm.type != 0) {
                        if (j == maxB) {
                            so = rtm_v3(0, 0, 0);
                            repeat_fixed();
                            finish_sample();
                        } else {
                            ++j;
                            phase = PREP;
                        }
                    } else {
                        so = rtm_scale(so, bm.rough);
                        repeat_fixed();
                        finish_sample();
                    }
                } else {
                    phase = SUN;   // escaped: shadow ray towards the sun (Raytracing.cl:115-124)
                    // unlit sun (FrameParams::sun_skip): the shadow ray cannot change the sample; it is not
                    // traced and the sun term below runs now with h, the bounce ray's miss
                    if (F.sun_skip) {
                    } else if (SUNC && fdb && sun_c != SUN_UNKNOWN) {
                        h.tri = sun_c;   // the first drawing bounce's shadow ray, traced in an earlier sample
                    } else {
                        start(T.o, C.sun);
                        T.any = F.sun_any != 0;
                        if (!tracing) continue;  // unreachable in practice (root box always hit from inside)
                    }
                }
            }
            if (phase == SUN && !tracing) {  // Raytracing.cl:125-137
                if (LOG && logme) {
                    const int hm = h.tri >= 0 ? __float_as_int(S.tri_shade[h.tri].w) : 0;
                    log_event(F, 2.0f, j, T.o, C.sun, h.tri >= 0 ? h.k : -1.0f, hm, so);
                }
                rtm_f3 sunLight = rtm_v3(0, 0, 0);
                if (COUNT) c.sun++;
                if (SUNC && fdb) sun_c = h.tri;
                const Mat cm = load_mat(S.mat, __float_as_int(S.tri_shade[tri].w));
                if (h.tri < 0 && cm.type != 3) sunLight = rtm_v3(e3, e3, e3);
                if (h.tri >= 0) {
                    const Mat sm = load_mat(S.mat, __float_as_int(S.tri_shade[h.tri].w));
                    if (sm.type == 3) sunLight = rtm_scale(sm.color, e3);
                }
                const rtm_f3 envLight = rtm_scale(sample_ibl_if<COUNT>(S, C, Bd, e4, c), e4);
                so = rtm_mul(so, rtm_add(sunLight, envLight));
                repeat_fixed();
                finish_sample();
            }
            // naiveGI loop heads (Raytracing.cl:46-79) until a ray is needed or the pixel is done
            while (phase == PREP) {
                const bool cam = j == 0;
                const rtm_f3 Ro = cam ? C.position : T.o, Rd = cam ? cd : T.d;
                const float k = cam ? kc : T.bk;
                if (j > maxB) {
                    repeat_fixed();
                    finish_sample();   // naiveGI's loop never entered (maxBounce < 0): the sample stays 1
                } else if (tri < 0) {
                    so = rtm_scale(rtm_mul(so, sample_ibl_if<COUNT>(S, C, Rd, e4, c)), e4);
                    repeat_fixed();
                    finish_sample();
                } else {
                    const float4 sh = S.tri_shade[tri];
                    const rtm_f3 n = xyz(sh);
                    const Mat cm = load_mat(S.mat, __float_as_int(sh.w));
                    if (cm.type == 0) {
                        so = rtm_scale(so, cm.rough);
                        repeat_fixed();
                        finish_sample();
                    } else {
                        const float4 f2 = S.tri_frame[3 * tri + 2];
                        const rtm_f3 nn = xyz(f2);
                        float invPdf = 0.0f;
                        rtm_f3 brdf = rtm_v3(0, 0, 0);
                        if (COUNT) count_event(c, cm.type);
                        if (PREFIX && F.fixed_point && cm.type != 3 && !drew && j > 0 && !pre && !(LOG && logme)) {
                            pre = true;   // the first bounce of the sample that draws, reached through glass only
                            pre_j = j; pre_tri = tri;
                            pre_so = so;
                            pre_o = T.o; pre_d = T.d; pre_k = T.bk;
                        }
                        fdb = SUNC && F.sun_cache && cm.type != 3 && !drew && !F.sun_skip && !(LOG && logme);
                        drew = drew || cm.type != 3;
                        if (cm.type != 3) {   // diffuse (1) or glossy (2): one sampler stream for both
                            if (!WIDE) ndraw += 2;
                            Bd = hemi_sample(cm.type == 1, n, S.tri_frame[3 * tri], S.tri_frame[3 * tri + 1], f2,
                                             &seed1, &seed0, &invPdf);
                            if (cm.type == 1) brdf = rtm_scale(cm.color, 1.0f / 3.14f);
                            else brdf = brdf_ggx(cm.color, cm.rough, rtm_scale(Rd, -1.0f), Bd, n);
                        } else {
                            Bd = Rd;
                            brdf = cm.color;
                            invPdf = 1.0f / rtm_fabs(rtm_dot(Bd, nn));
                        }
                        const rtm_f3 nd = dev_normalize(Rd);
                        const rtm_f3 Bo = rtm_v3(fmaf(nd.x, k, Ro.x), fmaf(nd.y, k, Ro.y), fmaf(nd.z, k, Ro.z));
                        // attenuation depends only on pre-trace values (Raytracing.cl:86-87): apply now
                        const float att = invPdf * rtm_fabs(rtm_dot(Bd, nn));
                        so = rtm_scale(rtm_mul(so, brdf), att);
                        phase = BOUNCE;
                        start(Bo, Bd);
                    }
                }
            }
        }

        // -- traversal rounds until at least F.resume_min lanes have no ray in flight --
        unsigned long long t_mid = 0;
        if (COUNT) {
            t_mid = clock64();
            if (lane == 0) c.cyc_shade += t_mid - t_iter;
        }
        // lanes that finished their tile (DONE) take no part in the threshold: it is resume_min / 64
        // of the lanes still rendering (all 64 until the pixel counters run dry)
        const unsigned long long alive = __ballot(phase != DONE);
        const int rthr = F.resume_min * __popcll(alive);
        // BVH2 item steps of single lanes are software-pipelined (fast_step_pipe: the next item's loads go
        // out before this item's leaf test; r05: C3 114.4 -> 110.5 ms, C4 282.7 -> 284.6 ms); the loads
        // for the first step of this round are issued here (a lane continuing its ray re-fetches its item)
        constexpr bool PIPE = STEP && !WIDE && TS == 1;
        ItemData D;
        if (RT_TOP_LEVELS && PIPE && !SMEM && S.root_ref >= 0) {
            // rays started this round (still at the root: a started ray steps at least once per round)
            const bool fresh = tracing && T.item == S.root_ref;
            if (__ballot(fresh) && !top_levels<COUNT, OVF>(S, T, fresh, nb, lst, c)) tracing = false;
        }
        if (PIPE && tracing) D = item_fetch<SMEM>(T.item, nb, tb, kstride);
        while (true) {
            if (tracing && (PIPE ? fast_step_pipe<COUNT, SMEM, OVF>(T, D, nb, tb, lst, kstride, c)
                            : TS > 1 ? team_step<COUNT, SMEM, OVF>(TS, T, boff, nb, tb, lst, kstride, c)
                            : WIDE ? (STEP ? wide_step<COUNT, OVF, WIDE == 2>(T, wnb, wlb, lst, c)
                                           : wide_round<COUNT, OVF>(T, wnb, wlb, lst, c))
                            : STEP ? fast_step<COUNT, SMEM, OVF>(S, T, nb, tb, lst, kstride, c)
                                   : fast_round<COUNT, SMEM, OVF>(S, T, nb, tb, lst, kstride, c)))
                tracing = false;
            const unsigned long long tr = __ballot(tracing);
            if (tr == 0 || 64 * __popcll(alive & ~tr) >= rthr) break;
        }
        if (COUNT && lane == 0) c.cyc_trav += clock64() - t_mid;
    }
    if (COUNT) {
        if (!team_leader) {   // a team's lanes repeat its pixel's shading and rays: counted once
            c.rays = 0; c.env = 0; c.diffuse = 0; c.glossy = 0; c.glass = 0; c.sun = 0; c.samples = 0;
        }
        unsigned long long v[NCOUNTS] = {c.nodes, c.tris, c.rays, c.env, c.dropped, c.wave_trav, c.wave_outer,
                                          c.cyc_shade, c.cyc_trav, c.boxes, c.diffuse, c.glossy, c.glass,
                                          c.sun, c.samples};
#pragma unroll
        for (int q = 0; q < NCOUNTS; ++q) {
            unsigned long long x = v[q];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
            if (lane == 0 && x) atomicAdd(&counts[q], x);
        }
    }
}

__global__ void gamma_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float p = fminf(in[i], 1.0f);
        out[i] = powf(p, 2.2f);
    }
}

// Output stage (FileManager.py:334-336 saveImg: (data*255).astype('uint8'); with gamma first the
// ImgProcessing.cl:1-10 kernel, as gamma_kernel above).  Four elements per thread: float4 in,
// one 32-bit word of bytes out.  v*255 rounds in fp32 like numpy's float32 product; the
// conversion truncates toward zero like numpy's cast for every v*255 in [0, 256) (rendered
// frames are clamped to [0, 1]); outside that range it saturates (NaN -> 0).
template <bool GAMMA>
__device__ __forceinline__ unsigned rgb8_byte(float v) {
    if (GAMMA) v = powf(fminf(v, 1.0f), 2.2f);
    const float x = v * 255.0f;
    return (unsigned)min(max((int)x, 0), 255);   // v_cvt_i32_f32 truncates, NaN -> 0
}

template <bool GAMMA>
__global__ void rgb8_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, int64_t n) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // group of 4 elements
    const int64_t i = 4 * q;
    if (i + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(in + i);
        const unsigned w = rgb8_byte<GAMMA>(v.x) | (rgb8_byte<GAMMA>(v.y) << 8) | (rgb8_byte<GAMMA>(v.z) << 16) |
                           (rgb8_byte<GAMMA>(v.w) << 24);
        *reinterpret_cast<unsigned*>(out + i) = w;
    } else {
        for (int64_t k = i; k < n; ++k) out[k] = (uint8_t)rgb8_byte<GAMMA>(in[k]);
    }
}

// FrameParams::walk_team = 0 (auto): lanes per pixel of the tree walk.  Host rule (one-pass tiles,
// and pass 1 of a pilot launch) from the tile's pixels per resident lane: teams of 4 at <= 1 pixel
// per lane (measured on row tiles, profiles/r03_tile_scaling.json: C3 1/8 tile 83 -> 63 ms, C4 1/8
// tile 355 -> 167 ms, C4 1/4 tile 330 -> 206 ms; at 4-8 pixels per lane teams cost 1.3-2.1x).
inline int auto_walk_team(int64_t nloc, int64_t lanes) { return nloc <= lanes ? 4 : 1; }

// Device rule (pass 2 of a pilot launch): pass 1 finished every pixel whose samples draw nothing
// (fixed_point: sky pixels), so the pixels left, u per resident lane, are what pass 2 has to spread:
// teams of 4 at u <= 1/2, of 2 at u <= 1, else one lane per pixel (r03: C4 1/2 tile u = 0.9, teams
// of 2 323 vs 348 / 372 ms with 1 / 4 lanes; C3 1/2 tile u = 1.9, one lane 87 vs 106 ms).
__global__ void pilot_team_count_kernel(const uint32_t* __restrict__ cost, int64_t n, unsigned* __restrict__ left) {
    unsigned k = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        k += cost[i] != 0u;
    for (int off = 32; off > 0; off >>= 1) k += __shfl_down(k, off, 64);
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(left, k);
}

// spec: with speculation available (FrameParams::spec < 0, auto) the same thresholds pick trails instead of
// teams: 8 trails per pixel at u <= 1/4 per lane, 4 at u <= 1/2, 2 at u <= 1 (r04, 1/8 and 1/4 row tiles:
// C4 1/8 u ~ 0.23 per lane: 8 trails 82.1 ms, 4 trails 91.0 (85 on another box), teams 109, 2 trails 137;
// C3 1/8 u ~ 0.47: 2 / 4 / 8 trails 36.1 / 35.0 / 41.7 ms, teams 50.7; C3 1/4 u ~ 0.93: 2 trails 53.8,
// 4 trails 58.1-61.6, teams 66.8; whole frames (u ~ 1.8 C4, ~3.7 C3): 2 trails 302 / 151 vs one lane 300 /
// 125 ms), encoded kSpecPick + trails
__global__ void pilot_team_pick_kernel(const unsigned* __restrict__ left, int64_t lanes, int spec, int* __restrict__ ts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t u4 = 4 * (int64_t)*left;   // 4 u lanes
        const int k = u4 <= 2 * lanes ? 4 : u4 <= 4 * lanes ? 2 : 1;
        *ts = (spec && k > 1) ? kSpecPick + (u4 <= lanes ? 8 : k) : k;
    }
}

// ---- the kernel table of this translation unit: every instantiation it holds, by key ----
// rt_kernels.hip holds the one-shot kernels (product, instrumented, logging), rt_accum.hip the adds' and
// rt_adaptive.hip the listed adds' (product only).  The product kernels' instruction streams move with their
// module's contents: a row added here is a change to every kernel of the module.
#ifdef RT_ACCUM_TU
constexpr int kTuAcc = RT_ACCUM_TU;
#else
constexpr int kTuAcc = 0;
#endif
struct KernelRow {
    KernelKey key;
    const void* fn;
};
// A row's key is made from the template arguments that name its kernel: the two cannot disagree.
template <int TRAV, bool COUNT, bool LOG, bool SMEM, bool OVF, int BRUTE_>
KernelRow render_row() {
    // (BRUTE_'s bits above kBruteLean are the key's primary: 1 kBrutePrimary, 2 kBrutePrepass)
    return {KernelKey{TRAV, COUNT, LOG, SMEM, OVF, 0, 1, 0, BRUTE_ & (kBrutePrimary - 1), 1, kTuAcc, BRUTE_ / kBrutePrimary},
            (const void*)render_kernel<TRAV, COUNT, LOG, SMEM, OVF, BRUTE_, kTuAcc>};
}
template <bool COUNT, bool LOG, bool SMEM, bool OVF, bool STEP, int WIDE, int TS>
KernelRow walk_row() {
    return {KernelKey{TRAV_FAST, COUNT, LOG, SMEM, OVF, 1, STEP, WIDE, 0, TS, kTuAcc},
            (const void*)render_resume_kernel<COUNT, LOG, SMEM, OVF, STEP, WIDE, TS, kTuAcc>};
}
// The module holds its kernels in the order this file first names them -- the order of the rows -- and the product
// kernels' code moves with that order too (tools/code_object_diff.py shows it).  Hence this order:
// what the product and the instrumented kernels both have, the one-lane item-step walk and REF ...
template <bool COUNT>
void head_rows(std::vector<KernelRow>& t) {
    t.push_back(walk_row<COUNT, false, false, false, true, 0, 1>());
    t.push_back(render_row<TRAV_REF, COUNT, false, false, false, 0>());
}
// ... the 4-wide walk in rounds, the plain tree walk, the wide item steps origin-folded and exact ...
template <bool COUNT, bool OVF>
void wide_rows(std::vector<KernelRow>& t) {
    t.push_back(walk_row<COUNT, false, false, OVF, false, 1, 1>());
    t.push_back(render_row<TRAV_FAST, COUNT, false, false, OVF, 0>());
    t.push_back(walk_row<COUNT, false, false, OVF, true, 2, 1>());
    t.push_back(walk_row<COUNT, false, false, OVF, true, 1, 1>());
}
// ... the item-step teams of one stack / staging form
template <bool COUNT, bool SMEM, bool OVF>
void team_rows(std::vector<KernelRow>& t) {
    t.push_back(walk_row<COUNT, false, SMEM, OVF, true, 0, 2>());
    t.push_back(walk_row<COUNT, false, SMEM, OVF, true, 0, 4>());
    t.push_back(walk_row<COUNT, false, SMEM, OVF, true, 0, 8>());
}
// ... and the staged walks, the teams, the BVH2 walk in rounds, brute force lock-step, in teams and sliced.
// Product only: the clustered loop (3) and the refill forms (COUNT and LOG carry the threshold without the flag).
template <bool COUNT>
void engine_rows(std::vector<KernelRow>& t) {
    wide_rows<COUNT, true>(t);
    wide_rows<COUNT, false>(t);
    t.push_back(walk_row<COUNT, false, true, false, true, 0, 1>());
    t.push_back(render_row<TRAV_FAST, COUNT, false, true, false, 0>());
    team_rows<COUNT, true, false>(t);
    t.push_back(walk_row<COUNT, false, false, true, true, 0, 1>());
    team_rows<COUNT, false, true>(t);
    team_rows<COUNT, false, false>(t);
    t.push_back(walk_row<COUNT, false, true, false, false, 0, 1>());
    t.push_back(walk_row<COUNT, false, false, true, false, 0, 1>());
    t.push_back(walk_row<COUNT, false, false, false, false, 0, 1>());
    t.push_back(render_row<TRAV_FAST, COUNT, false, false, false, 1>());
    if constexpr (!COUNT) t.push_back(render_row<TRAV_FAST, COUNT, false, false, false, 3>());
    t.push_back(render_row<TRAV_FAST, COUNT, false, false, false, 2>());
    if constexpr (!COUNT) t.push_back(render_row<TRAV_FAST, COUNT, false, false, false, 3 | kBruteSliced>());
    t.push_back(render_row<TRAV_FAST, COUNT, false, false, false, 1 | kBruteSliced>());
    if constexpr (!COUNT) {
        t.push_back(render_row<TRAV_FAST, COUNT, false, false, false, 3 | kBruteSliced | kBruteRefill>());
        t.push_back(render_row<TRAV_FAST, COUNT, false, false, false, 1 | kBruteSliced | kBruteRefill>());
        t.push_back(render_row<TRAV_FAST, COUNT, false, false, false, 3 | kBruteRefill>());
        t.push_back(render_row<TRAV_FAST, COUNT, false, false, false, 1 | kBruteRefill>());
    }
}
// ... and, last, the lean forms of the one-lane brute-force product kernels (one-shot frames only)
template <int LOOP>
void lean_rows(std::vector<KernelRow>& t) {
    if constexpr (RT_SHADE_ROWS && !kTuAcc) {
        t.push_back(render_row<TRAV_FAST, false, false, false, false, LOOP | kBruteLean>());
        t.push_back(render_row<TRAV_FAST, false, false, false, false, LOOP | kBruteSliced | kBruteLean>());
        t.push_back(render_row<TRAV_FAST, false, false, false, false, LOOP | kBruteSliced | kBruteRefill | kBruteLean>());
        t.push_back(render_row<TRAV_FAST, false, false, false, false, LOOP | kBruteRefill | kBruteLean>());
    }
}
// ... and behind them the lean sliced kernels that start every job from a record, and the pre-pass that writes the
// records (option "brute_primary")
template <int LOOP>
void primary_rows(std::vector<KernelRow>& t) {
    if constexpr (RT_SHADE_ROWS && !kTuAcc) {
        t.push_back(render_row<TRAV_FAST, false, false, false, false, LOOP | kBruteSliced | kBruteLean | kBrutePrimary>());
        t.push_back(render_row<TRAV_FAST, false, false, false, false, LOOP | kBruteSliced | kBruteRefill | kBruteLean | kBrutePrimary>());
        t.push_back(render_row<TRAV_FAST, false, false, false, false, LOOP | kBrutePrepass>());
    }
}

// ---- test hooks (rt_debug.h): device evaluation of the numerics contract and of
// single rays through either traversal ----
__global__ void debug_math_kernel(int fn, const float* __restrict__ x, const float* __restrict__ y,
                                  float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = 0.0f;
    switch (fn) {
        case 0: r = rtm_sin(x[i]); break;
        case 1: r = rtm_cos(x[i]); break;
        case 2: r = rtm_tan(x[i]); break;
        case 3: r = rtm_asin(x[i]); break;
        case 4: r = rtm_acos(x[i]); break;
        case 5: r = rtm_atan2(x[i], y[i]); break;
        case 6: r = sqrtf(x[i]); break;
        case 7: r = x[i] / y[i]; break;
        case 8: r = mt_recip(x[i]); break;   // the Moller-Trumbore reciprocal of the FAST walks
        case 9: r = dev_sqrt(x[i]); break;   // the shading's sqrtf
        case 10: r = dev_inv_sqrt(x[i]); break;   // dev_normalize's scale, 1.0f / sqrtf
        case 11: r = dev_recip(x[i]); break;   // the kernels' 1.0f / x (ray inverses, GGX)
        default: break;
    }
    out[i] = r;
}

template <int TRAV>
__global__ void __launch_bounds__(256) debug_trace_kernel(DevScene S, const float* __restrict__ rays,
                                                          float* __restrict__ out, int64_t n) {
    extern __shared__ int lds_stack[];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    Cnt c{};
    const float* r = rays + 6 * t;
    const Hit h = trace<TRAV, false>(S, S.nodes, S.tri_fast, rtm_v3(r[3], r[4], r[5]), rtm_v3(r[0], r[1], r[2]),
                                     lds_stack + threadIdx.x, blockDim.x, lane_stack(S, lds_stack), c);
    out[2 * t + 0] = h.k;
    out[2 * t + 1] = (float)h.tri;
}

}  // namespace

// rt_accum.hip compiles this file again with RT_ACCUM_TU defined (1): that translation unit holds the ACC
// instantiations of the kernels (through launch_accum) and none of the other entry points, so the code
// object of this one -- every one-shot kernel -- is built from exactly what it was built from without them
// (rt_adaptive.hip, RT_ACCUM_TU 2, does the same for the listed instantiations: launch_accum_listed, below)
#ifndef RT_ACCUM_TU
// the last launch_pick of any of the three translation units (rt_debug_last_launch: which kernel a test launched)
static std::mutex g_note_mu;
static LaunchNote g_note{};
void note_launch(const LaunchNote& n) {
    std::lock_guard<std::mutex> g(g_note_mu);
    g_note = n;
}
LaunchNote last_launch() {
    std::lock_guard<std::mutex> g(g_note_mu);
    return g_note;
}

int64_t resident_blocks(const void* fn, int block, size_t lds, int max_waves, hipError_t* err) {
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t e = fn ? hipGetDevice(&dev) : hipErrorInvalidDeviceFunction;   // a kernel that is not built
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) {
        // (a context may hold devices of different kinds)
        struct Occ { int dev; const void* fn; int block; size_t lds; int per_cu; };
        static std::mutex mu;
        static std::vector<Occ> seen;
        std::lock_guard<std::mutex> g(mu);
        for (const Occ& o : seen)
            if (o.dev == dev && o.fn == fn && o.block == block && o.lds == lds) per_cu = o.per_cu;
        if (per_cu == 0) {
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, lds);
            if (seen.size() >= 1024) seen.clear();   // (a process that renders very many scenes: lds varies)
            if (e == hipSuccess) seen.push_back({dev, fn, block, lds, per_cu});
        }
    }
    if (e != hipSuccess) {
        *err = e;
        return 0;
    }
    // blocks per CU for at most max_waves waves per SIMD (4 SIMDs per CU)
    const int cap_cu = max_waves > 0 ? std::max(1, max_waves * 4 * 64 / block) : INT_MAX;
    return (int64_t)std::max(1, cus) * std::max(1, std::min(per_cu, cap_cu));
}


hipError_t launch_debug_math(int fn, const float* x, const float* y, float* out, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(debug_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fn, x, y, out, n);
    return hipGetLastError();
}

namespace {
// The logging kernels' rows of the kernel table (below): REF and the plain walk with and without overflow (the two
// resumable walks are never launched -- a log runs the plain walk -- but part of this module since the logging
// launches named them).  They stand here, before launch_debug_trace, because the module holds its kernels in the
// order this file first names them, and that order is part of the one-shot kernels' code (kernel_table).
void log_rows(std::vector<KernelRow>& t) {
    t.push_back(walk_row<false, true, false, false, true, 0, 1>());
    t.push_back(render_row<TRAV_REF, false, true, false, false, 0>());
    t.push_back(walk_row<false, true, false, true, true, 0, 1>());
    t.push_back(render_row<TRAV_FAST, false, true, false, true, 0>());
    t.push_back(render_row<TRAV_FAST, false, true, false, false, 0>());
}
}  // namespace

hipError_t launch_ibl_sum(const uchar4* rgba, int w, int h, uint32_t* sum, hipStream_t stream) {
    const int64_t n = (int64_t)(w + 1) * (h + 1);
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 65536);
    hipLaunchKernelGGL(ibl_sum_kernel, dim3(grid), dim3(256), 0, stream, rgba, w, h, sum);
    return hipGetLastError();
}

hipError_t launch_prep_frames(const DevScene& sc, float4* frame, hipStream_t stream) {
    if (sc.ntri <= 0) return hipSuccess;
    hipLaunchKernelGGL(prep_frames_kernel, dim3((unsigned)((sc.ntri + 255) / 256)), dim3(256), 0, stream, sc.tri_shade,
                       sc.mat, sc.ntri, frame);
    return hipGetLastError();
}

hipError_t launch_debug_trace(const DevScene& sc, int traversal, const float* rays, float* out, int64_t n,
                              hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int block = 128;
    // not a persistent grid: the whole FAST stack lives in LDS (no overflow buffer sized for this grid)
    DevScene s2 = sc;
    s2.stack_lds = sc.depth > 0 ? sc.depth : 1;
    s2.stack_ovf = nullptr;
    const size_t lds = stack_lds_bytes(s2, traversal == TRAV_REF ? TRAV_REF : TRAV_FAST, block);
    if (traversal == TRAV_REF)
        hipLaunchKernelGGL(debug_trace_kernel<TRAV_REF>, dim3((unsigned)((n + block - 1) / block)), dim3(block), lds,
                           stream, s2, rays, out, n);
    else
        hipLaunchKernelGGL(debug_trace_kernel<TRAV_FAST>, dim3((unsigned)((n + block - 1) / block)), dim3(block), lds,
                           stream, s2, rays, out, n);
    return hipGetLastError();
}

// A small tree-walk scene is staged in LDS (SMEM kernels).  Those kernels keep the whole stack in LDS too:
// they have no spill code, and the staged arrays start right behind stack_lds entries per lane, so an
// entry past stack_lds would overwrite the staged nodes.  Hence only trees no deeper than stack_lds: a
// small but deep tree (a 40-level chain, or any tree with option "stack_lds" below its depth) walks the
// arrays in global memory with the overflow buffer instead.
static bool stage_in_lds(const DevScene& sc) {
    const size_t scene_bytes = (size_t)(kNodeF4 * sc.nnodes + 3 * sc.ntri) * sizeof(float4);
    return sc.ntri > 0 && sc.nbrute == 0 && scene_bytes <= kLdsSceneMax && sc.stack_lds >= sc.depth;
}

KernelKey choose_kernel(const DevScene& sc, const FrameParams& fp, int traversal, bool count, bool log, int acc,
                        int block) {
    KernelKey k{traversal, count, log, /*smem*/ 0, /*ovf*/ 0, /*resume*/ 0, /*step*/ 1, /*wide*/ 0, /*brute*/ 0, /*ts*/ 1, acc};
    if (traversal == TRAV_REF) return k;
    k.ovf = sc.nbrute == 0 && sc.stack_lds < sc.depth;
    if (log) return k;   // a log runs the plain walk (on a brute-force scene: its loop over the global records)
    if (sc.ntri > 0 && sc.nbrute == 0 && fp.resume_min > 0) {
        k.resume = 1;
        if (fp.wide && sc.wnodes && !stage_in_lds(sc)) {
            // the wide walk takes item steps unless rounds are asked for (C5: 1,181 vs 1,035 Msamples/s);
            // the item steps dequantise origin-folded (2) when every ray origin of the frame is within
            // the bound the builder's gap covers: hit points always are, the camera is checked here
            // (each coordinate compared on its own: false for a NaN in any of them, which a std::max over the
            // three would drop from its second operand)
            const bool cam_in = std::fabs(fp.cam[0]) <= sc.wdq_omax && std::fabs(fp.cam[1]) <= sc.wdq_omax &&
                                std::fabs(fp.cam[2]) <= sc.wdq_omax;
            k.step = fp.step != 2;
            k.wide = (k.step && fp.wdq != 0 && sc.wdq_omax > 0.0f && cam_in) ? 2 : 1;
            return k;
        }
        k.step = fp.step == 1 || (fp.step == 0 && (size_t)sc.nnodes * kNodeF4 * 16 <= kStepMaxBytes);
        k.smem = stage_in_lds(sc);   // (never with ovf: staged trees are no deeper than stack_lds)
        return k;
    }
    // brute force stages the scene in LDS: only while two blocks still fit a CU
    if (sc.ntri > 0 && sc.nbrute > 0 && std::max(brute_lds_bytes(sc, block, true), brute_lds_bytes(sc, block, false)) <= 80 * 1024) k.brute = 1;
    else k.smem = stage_in_lds(sc);
    return k;
}

#endif  // !RT_ACCUM_TU

#if RT_CHAIN_STAMPS
namespace {
// the stamps' sums (kStampN words), shared by every product launch of this translation unit
unsigned long long* chain_stamp_buffer() {
    static unsigned long long* p = [] {
        unsigned long long* q = nullptr;
        if (hipMalloc(&q, kStampN * sizeof(unsigned long long)) != hipSuccess) return (unsigned long long*)nullptr;
        if (hipMemset(q, 0, kStampN * sizeof(unsigned long long)) != hipSuccess) return (unsigned long long*)nullptr;
        return q;
    }();
    return p;
}
}  // namespace
#ifndef RT_ACCUM_TU
// tools/chain_stamps.py: the sums since the last call (the one-shot frames' launches), then zeroed; blocking
extern "C" __attribute__((visibility("default"))) int rt_debug_chain_stamps(unsigned long long out[kStampN]) {
    unsigned long long* p = chain_stamp_buffer();
    if (!p || hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpy(out, p, kStampN * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    return hipMemset(p, 0, kStampN * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif
#endif

namespace {
// the instantiation a key names; nullptr: not built
const void* kernel_fn(const KernelKey& k) {
    static const std::vector<KernelRow> table = [] {
        std::vector<KernelRow> t;
#ifndef RT_ACCUM_TU
        log_rows(t);
        head_rows<true>(t);
        head_rows<false>(t);
        engine_rows<true>(t);
#else
        head_rows<false>(t);
#endif
        engine_rows<false>(t);
        lean_rows<3>(t);
        lean_rows<1>(t);
        primary_rows<3>(t);
        primary_rows<1>(t);
        return t;
    }();
    for (const KernelRow& r : table)
        if (r.key == k) return r.fn;
    return nullptr;
}

// One pass: the engine choose_kernel picked, refined by the tile's rules in their order, each going by the resident
// lanes of the kernel picked so far; then a persistent grid (pixels are handed out by d_work) of the kernel named
hipError_t launch_pick(const DevScene& sc, const FrameParams& fp, KernelKey k, int block, float* d_out,
                       unsigned long long* d_counts, unsigned int* d_work, hipStream_t stream) {
    if (fp.nloc <= 0) return hipSuccess;
    const bool brute = k.brute != 0, product = !k.count && !k.log, listed = k.acc == kAccListed;
    // (a brute-force launch: the rules below go by the team kernel's bytes, as they did when every brute-force
    // kernel staged its tables; the launch takes the bytes of the kernel they end at)
    size_t lds = (brute ? brute_lds_bytes(sc, block, true) : stack_lds_bytes(sc, k.trav, block)) +
                 (k.smem ? staged_scene_bytes(sc) : 0);
    hipError_t e = hipSuccess;
    // blocks the device keeps resident of the kernel k names now, at most max_waves waves per SIMD
    auto resident = [&](int max_waves) { return resident_blocks(kernel_fn(k), block, lds, max_waves, &e); };
    // clustered scenes (DevScene::ncluster > 0) run the one-lane product kernel with the clustered loop (3); the
    // instrumented build and every other scene keep the lock-step loop over brute_box (1).
    // auto: only tiles with at least one pixel per resident lane.  Measured on C2: the whole
    // frame (3.2 pixels per lane) 7.29 -> 7.02 ms, the 1/8 tile (0.4 per lane: half-empty waves that wait on
    // the LDS round trips of the item batches instead of on VALU issue) 2.14 -> 2.23 ms
    if (brute && product && sc.ncluster > 0 && !((sc.host_flags & kHostClusterAuto) && fp.nloc < resident(0) * block)) k.brute = 3;
    const int64_t lanes = resident(fp.max_waves) * block;
    if (e != hipSuccess) return e;
    FrameParams f = fp;
    // sample slices of the one-lane brute-force kernels (rt_api.hip setup_slices: fp.slices = K, or -K for K
    // on auto, decided here where the resident lanes are known: rt_slices.h brute_slice_launch): one-pass
    // launches only, and no teams -- a set slice count keeps a tile the team rule would take on single lanes.
    // The sliced kernels read FrameParams::slices as K | tail << 8 (a set slice count slices every pixel, auto
    // only the tile's last pixels), 0 for an unsliced launch; the resumable walk reads fp.slices as it is
    int bslices = 0;
    if (brute && !listed && fp.pass == 0 && fp.team <= 1 && fp.slice_state && fp.slice_ready &&
        sc.ntri + 2 < 65536 && fp.npix <= INT_MAX)
        bslices = brute_slice_launch(fp.slices, fp.nloc, lanes);
    if (!k.resume) f.slices = bslices;
    // brute-force teams: a tile with fewer pixels than the device has lanes (a row slice of a multi-GPU frame)
    // gives each pixel 4 lanes that split its box tests when it fills at most a quarter of them.  Measured on
    // C2 tiles (one MI355X, 96-VGPR kernel: 327,680 resident lanes): a 1/8 tile (131k pixels) is fastest with
    // single lanes (2.23 vs 2.29 ms with pairs), a 1/16 tile with teams of 4 (1.67 vs 1.88 with pairs, 2.28
    // single).  (A listed add: the list's length is known on the device only -- one lane per pixel unless
    // teams are set; the same for the walk's teams below.)
    f.team = !brute ? 1 : bslices ? 1 : fp.team;
    if (f.team == 0) f.team = (!listed && fp.nloc * 4 <= lanes) ? 4 : 1;
    // team walk (render_resume_kernel TEAM): BVH2 item steps only; walk_team, 0 = auto (auto_walk_team;
    // pass 2 of a pilot launch: the size pilot_team_pick_kernel chose, launch_render)
    f.walk_team = 1;
    if (k.resume && k.step && !k.wide && !k.log) {
        f.walk_team = fp.walk_team ? fp.walk_team : listed ? 1 : auto_walk_team(fp.nloc, lanes);
        if (f.walk_team != 2 && f.walk_team != 4 && f.walk_team != 8) f.walk_team = 1;
    }
    // the refill threshold of the one-lane brute-force kernels (fp.refill: the option; f.refill: R, or 0)
    f.refill = (brute && f.team <= 1) ? brute_refill_launch(fp.refill, fp.nloc, lanes) : 0;
    // teams, slices and the product kernels' refill threshold are instantiations of their own
    k.ts = f.walk_team;
    if (brute && f.team > 1) k.brute = 2;
    else if (brute) k.brute |= (bslices ? kBruteSliced : 0) | (product && f.refill > 1 ? kBruteRefill : 0);
    // ... and so is the lean loop of an all-diffuse one-shot frame (rt_internal.h: the rule; one-shot kernels only, so
    // rt_accum.hip's and rt_adaptive.hip's translation units hold none)
    if (RT_SHADE_ROWS && !kTuAcc && brute_lean_kernel(k, f.team) && brute_lean_frame(sc.host_flags, f)) k.brute |= kBruteLean;
    // ... and of a lean sliced launch, the loop that starts every job from the record a pre-pass wrote (below; option
    // "brute_primary" not 0, kHostPrimary).  Lean and sliced only: the records' buffer is then there (setup_slices),
    // and every other launch keeps its kernel and gains no launch
    if ((k.brute & kBruteLean) && bslices && (sc.host_flags & kHostPrimary)) k.primary = 1;
    if (brute && f.team <= 1) lds = brute_lds_bytes(sc, block, false);
    const void* fn = kernel_fn(k);
    // the grid stays within what the device keeps resident (not that the slices' hand-off needs it: a job is only
    // held by a running wave, and a pixel's slice k is taken before its slice k + 1)
    const int64_t need = (fp.nloc * f.team * f.walk_team + block - 1) / block;
    const int64_t grid = std::min(need, resident(fp.max_waves));
    if (e != hipSuccess) return e;
    // the samples-done words of the tile's pixels (the tree walk's are zeroed by setup_slices)
    // (a launch with a pre-pass: the pre-pass writes them)
    if (bslices && !k.primary) e = hipMemsetAsync(f.slice_ready, 0, (size_t)fp.nloc * sizeof(uint32_t), stream);
    const LaunchConst* lc = nullptr;
    if (e == hipSuccess) e = setup_work_block(f, d_work, stream, &lc);
    if (e != hipSuccess) return e;
    const int shell = (k.brute & 3) == 3 && sc.shell != 0;
    note_launch({k, f.team, f.walk_team, f.slices, f.refill, grid, lds, shell, shell && sc.near_floor != 0.0f,
                 shell && (sc.host_flags & kHostQuad) != 0, shell && (sc.host_flags & kHostDirect) != 0, k.primary});
#if RT_CHAIN_STAMPS
    if (!d_counts) d_counts = chain_stamp_buffer();   // (nullptr when the allocation failed: the kernel then adds nothing)
#endif
    DevScene a0 = sc;
    void* args[] = {&a0, &f, &d_out, &d_counts, &d_work, &lc};
    if (k.primary) {
        // the pre-pass, behind make_const_kernel on the launch's stream and before the loop kernel: the same arguments
        // and LDS (it stages what the loop kernel stages), a resident grid that strides over the tile's pixels
        KernelKey kp = k;
        kp.brute &= 3;
        kp.primary = 2;
        const void* fpre = kernel_fn(kp);
        const int64_t gpre = std::min((fp.nloc + block - 1) / block, resident_blocks(fpre, block, lds, fp.max_waves, &e));
        if (e != hipSuccess) return e;
        e = hipLaunchKernel(fpre, dim3((unsigned)gpre), dim3(block), args, lds, stream);
        if (e != hipSuccess) return e;
    }
    return hipLaunchKernel(fn, dim3((unsigned)grid), dim3(block), args, lds, stream);
}

}  // namespace

#ifndef RT_ACCUM_TU
hipError_t launch_debug_log(const DevScene& sc, const FrameParams& fp, int traversal, float* d_out,
                            unsigned int* d_work, hipStream_t stream) {
    return launch_pick(sc, fp, choose_kernel(sc, fp, traversal, false, true, 0, 64), 64, d_out, nullptr, d_work, stream);
}

// ---- two-pass ordering (FrameParams::pass): pilot costs -> pixel order, most expensive first ----
// Pixels are ordered in chunks of `chunk` consecutive tile pixels: the chunks by their summed pilot
// cost, the pixels of a chunk in tile order.  The tree walk orders single pixels (its lanes diverge
// anyway); the brute-force path would need chunks of a wave (64) to keep neighbouring lanes on
// neighbouring pixels -- its box loop and shading branches pay per wave -- and then gains nothing,
// so it runs one pass unless asked.
constexpr int kCostBins = 256;

__global__ void pilot_chunk_kernel(const uint32_t* __restrict__ cost, int64_t nfull, int chunk,
                                   uint32_t* __restrict__ ccost) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nfull; c += (int64_t)gridDim.x * blockDim.x) {
        uint32_t t = 0;
        for (int k = 0; k < chunk; ++k) t += cost[c * chunk + k];
        ccost[c] = t;
    }
}

// (the minimum in 64 bits: scale reaches 2^24, so a 32-bit cost's scaled value reaches 2^40, and cut to a word
// before the minimum it would land in a low bin instead of saturating -- no render's cost gets there, a chunk
// traces about `top` rays at most, but rt_debug_pilot_order takes any word)
__device__ __forceinline__ uint32_t cost_bin(uint32_t v, uint32_t scale, uint32_t maxbin) {
    const uint64_t b = ((uint64_t)v * scale) >> 16;
    return b < maxbin ? (uint32_t)b : maxbin;
}

// Stable counting sort of the chunks by cost bin (descending bins, tile order within a bin, so the
// pixels of one bin keep their raster order and a wave's lanes stay on nearby pixels), over segments
// of kSortSeg chunks: per-segment histograms (bin-major), their per-bin exclusive scan, the bin
// offsets, then each chunk's place = bin offset + segment offset + its rank among the segment's
// chunks of the same bin.
constexpr int kSortSeg = kCostBins;

__global__ void pilot_seg_hist_kernel(const uint32_t* __restrict__ ccost, int64_t n, int64_t nseg, uint32_t scale,
                                      uint32_t maxbin, uint32_t* __restrict__ seghist) {
    __shared__ uint32_t h[kCostBins];
    const int64_t seg = blockIdx.x;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t q = seg * kSortSeg + threadIdx.x;
    if (q < n) atomicAdd(&h[cost_bin(ccost[q], scale, maxbin)], 1u);
    __syncthreads();
    seghist[threadIdx.x * nseg + seg] = h[threadIdx.x];
}

// one block per bin: exclusive scan of the bin's row of seghist in place, the row total to total[bin]
__global__ void pilot_seg_scan_kernel(uint32_t* __restrict__ seghist, int64_t nseg, uint32_t* __restrict__ total) {
    __shared__ uint32_t t[kCostBins];
    uint32_t* row = seghist + (int64_t)blockIdx.x * nseg;
    const int i0 = threadIdx.x;
    uint32_t carry = 0;
    for (int64_t base = 0; base < nseg; base += kCostBins) {
        const int64_t i = base + i0;
        const uint32_t v = i < nseg ? row[i] : 0u;
        t[i0] = v;
        __syncthreads();
        for (int off = 1; off < kCostBins; off <<= 1) {
            const uint32_t a = i0 >= off ? t[i0 - off] : 0u;
            __syncthreads();
            t[i0] += a;
            __syncthreads();
        }
        if (i < nseg) row[i] = carry + t[i0] - v;
        carry += t[kCostBins - 1];
        __syncthreads();
    }
    if (i0 == 0) total[blockIdx.x] = carry;
}

// offs[b] = number of chunks in bins above b (descending cost order); one block of kCostBins threads
__global__ void pilot_scan_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ offs) {
    __shared__ uint32_t t[kCostBins];
    const int b = threadIdx.x;
    t[b] = hist[b];
    __syncthreads();
    uint32_t above = 0;
    for (int c = b + 1; c < kCostBins; ++c) above += t[c];
    offs[b] = above;
}

__global__ void pilot_seg_scatter_kernel(const uint32_t* __restrict__ ccost, int64_t n, int64_t nseg, uint32_t scale,
                                         uint32_t maxbin, const uint32_t* __restrict__ seghist,
                                         const uint32_t* __restrict__ offs, uint32_t* __restrict__ corder) {
    __shared__ uint32_t bins[kSortSeg];
    const int64_t seg = blockIdx.x;
    const int64_t q = seg * kSortSeg + threadIdx.x;
    const uint32_t b = q < n ? cost_bin(ccost[q], scale, maxbin) : 0xffffffffu;
    bins[threadIdx.x] = b;
    __syncthreads();
    if (q >= n) return;
    uint32_t rank = 0;
    for (int j = 0; j < (int)threadIdx.x; ++j) rank += bins[j] == b ? 1u : 0u;
    corder[offs[b] + seghist[(int64_t)b * nseg + seg] + rank] = (uint32_t)q;
}

// pixel order: the full chunks in cost order, then the last partial chunk (if any) in place
__global__ void pilot_expand_kernel(const uint32_t* __restrict__ corder, int64_t nfull, int chunk, int64_t nloc,
                                    uint32_t* __restrict__ order) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nloc; q += (int64_t)gridDim.x * blockDim.x)
        order[q] = q < nfull * chunk ? corder[q / chunk] * (uint32_t)chunk + (uint32_t)(q % chunk) : (uint32_t)q;
}

// One pass of a one-shot frame: choose the engine, then launch_pick
static hipError_t launch_pass(const DevScene& sc, const FrameParams& fp, int traversal, int block, float* d_out,
                              unsigned long long* d_counts, unsigned int* d_work, hipStream_t stream) {
    const KernelKey k = choose_kernel(sc, fp, traversal, d_counts != nullptr, false, 0, block);
    return launch_pick(sc, fp, k, block, d_out, d_counts, d_work, stream);
}

// Two passes (fp.pilot > 0, product launches only): the first fp.pilot samples of every pixel,
// then the rest of each pixel in descending order of the rays its (chunk's) pilot samples traced.  The
// frame ends when its last-started pixels finish; started last, the cheapest pixels make that tail
// short.  Every pixel's samples run in the same order as in one pass, so the frame is bit-identical.
// The order's chunk and bins as the launch takes them from FrameParams::pilot_chunk / pilot_levels
static int pilot_chunk_of(int chunk) { return std::max(chunk, 1); }
static int pilot_levels_of(int levels) { return std::min(std::max(levels, 2), kCostBins); }

// The ordering launches of a two-pass launch: chunk sums, the segmented counting sort, the expansion to pixels
hipError_t launch_pilot_order(const uint32_t* cost, int64_t n, int chunk_, int levels_, int pilot, int max_bounce,
                              uint32_t* order, hipStream_t stream) {
    if (!cost || !order || n <= 0) return hipErrorInvalidValue;
    // scratch after the pixel order (rt_internal.h pilot_layout): bin totals | offs | chunk costs |
    // chunk order | segment histograms
    uint32_t* total = order + n;
    uint32_t* offs = total + kCostBins;
    const int chunk = pilot_chunk_of(chunk_);
    const int64_t nfull = n / chunk;
    const int64_t nseg = (nfull + kSortSeg - 1) / kSortSeg;
    uint32_t* ccost = offs + kCostBins;
    uint32_t* corder = ccost + nfull;
    uint32_t* seghist = corder + nfull;
    // `levels` cost bins over a chunk's rays up to 2 (maxBounce + 1) rays per pilot sample per pixel
    const int levels = pilot_levels_of(levels_);
    const uint64_t top = (uint64_t)chunk * pilot * 2u * (uint64_t)(std::max(max_bounce, 0) + 1);
    const uint32_t scale = (uint32_t)std::max<uint64_t>(1, ((uint64_t)levels << 16) / std::max<uint64_t>(top, 1));
    const uint32_t maxbin = (uint32_t)levels - 1;
    const unsigned gc = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nfull + 255) / 256, 2048));
    const unsigned gp = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
    if (nfull > 0) {
        hipLaunchKernelGGL(pilot_chunk_kernel, dim3(gc), dim3(256), 0, stream, cost, nfull, chunk, ccost);
        hipLaunchKernelGGL(pilot_seg_hist_kernel, dim3((unsigned)nseg), dim3(kSortSeg), 0, stream, ccost, nfull, nseg,
                           scale, maxbin, seghist);
        hipLaunchKernelGGL(pilot_seg_scan_kernel, dim3(kCostBins), dim3(kCostBins), 0, stream, seghist, nseg, total);
        hipLaunchKernelGGL(pilot_scan_kernel, dim3(1), dim3(kCostBins), 0, stream, total, offs);
        hipLaunchKernelGGL(pilot_seg_scatter_kernel, dim3((unsigned)nseg), dim3(kSortSeg), 0, stream, ccost, nfull,
                           nseg, scale, maxbin, seghist, offs, corder);
    }
    hipLaunchKernelGGL(pilot_expand_kernel, dim3(gp), dim3(256), 0, stream, corder, nfull, chunk, n, order);
    return hipSuccess;
}

// Pass 2's team size from the pixels pass 1 left unfinished (pilot_team_count_kernel, pilot_team_pick_kernel)
hipError_t launch_pilot_pick(const uint32_t* cost, int64_t n, int64_t lanes, int spec, unsigned* left, int* ts,
                             hipStream_t stream) {
    if (!cost || !left || !ts || n <= 0) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(left, 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    const unsigned gp = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(pilot_team_count_kernel, dim3(gp), dim3(256), 0, stream, cost, n, left);
    hipLaunchKernelGGL(pilot_team_pick_kernel, dim3(1), dim3(64), 0, stream, left, lanes, spec ? 1 : 0, ts);
    return hipSuccess;
}

hipError_t launch_render(const DevScene& sc, const FrameParams& fp, int traversal, int block, float* d_out,
                         unsigned long long* d_counts, unsigned int* d_work, hipStream_t stream, RenderPending* pend,
                         PilotNote* note) {
    if (note) *note = PilotNote{};
    if (fp.pilot <= 0 || fp.pass != 0 || d_counts || fp.spp <= fp.pilot || fp.nloc <= 0 || !fp.pilot_state)
        return launch_pass(sc, fp, traversal, block, d_out, d_counts, d_work, stream);
    FrameParams a = fp;
    a.pass = 1;
    hipError_t e = launch_pass(sc, a, traversal, block, d_out, nullptr, d_work, stream);
    if (e != hipSuccess) return e;
    e = launch_pilot_order(fp.pilot_cost, fp.nloc, fp.pilot_chunk, fp.pilot_levels, fp.pilot, fp.max_bounce,
                           const_cast<uint32_t*>(fp.pilot_order), stream);
    if (e != hipSuccess) return e;
    if (note) {
        note->two_pass = 1;
        note->nloc = fp.nloc;
        note->pilot = fp.pilot;
        note->chunk = pilot_chunk_of(fp.pilot_chunk);
        note->levels = pilot_levels_of(fp.pilot_levels);
    }
    FrameParams b = fp;
    b.pass = 2;
    // small tiles of the BVH2 walk: each pixel's remaining samples as speculative trails (rt_spec.hip):
    // a set number of trails, or (spec < 0) chosen on the device with the team size
    // (the walk rt_spec.hip continues is the BVH2 item-step resumable kernel, unstaged)
    const KernelKey wk = choose_kernel(sc, fp, traversal, false, false, 0, block);
    const bool spec_walk = wk.resume && wk.step && !wk.wide && !wk.smem;
    const bool spec_ok = traversal == TRAV_FAST && fp.spec != 0 && fp.spec_log && fp.pilot_draws && spec_walk;
    if (spec_ok && fp.spec > 0) return launch_spec(sc, b, block, d_out, d_work, stream);
    // (the brute-force kernels take their team size from the tile, launch_pick: no pick, no read-back)
    if (fp.walk_team == 0 && traversal == TRAV_FAST && sc.nbrute == 0) {
        // pass 2's team size from the pixels pass 1 left unfinished (pilot_team_pick_kernel)
        static_assert(kTeamOffset >= kGroups * kCounterStride && kTeamOffset + 8 <= kConstOffset, "work block layout");
        unsigned* left = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(d_work) + kTeamOffset);
        int* ts = reinterpret_cast<int*>(left + 1);
        int dev = 0, cus = 0;
        e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
        // resident lanes of the one-lane BVH2 walk: 4 waves per SIMD
        const int64_t lanes = (int64_t)std::max(cus, 1) * kWalkLanesPerCu;
        e = launch_pilot_pick(fp.pilot_cost, fp.nloc, lanes, spec_ok ? 1 : 0, left, ts, stream);
        if (e != hipSuccess) return e;
        if (note) note->lanes = lanes;
        // the pick is read back (pass 1 has to finish before pass 2 anyway) and exactly the kernel it names
        // is launched: 1, 2 or 4 lanes per pixel, or kSpecPick + T trails
        RenderPending local;
        RenderPending& P = pend ? *pend : local;
        int pick_stack = 1;
        if (!P.host_pick) {
            if (pend) return hipErrorInvalidValue;   // a deferred pass 2 needs the caller's (pinned) int
            P.host_pick = &pick_stack;               // pageable: this call waits itself
        }
        e = hipMemcpyAsync(P.host_pick, ts, sizeof(int), hipMemcpyDeviceToHost, stream);
        if (e != hipSuccess) return e;
        P.pick = true;
        P.b = b;
        P.spec_ok = spec_ok;
        if (pend) return hipSuccess;
        return launch_render_finish(sc, traversal, block, d_out, d_work, stream, P);
    }
    return launch_pass(sc, b, traversal, block, d_out, nullptr, d_work, stream);
}

hipError_t launch_render_finish(const DevScene& sc, int traversal, int block, float* d_out, unsigned int* d_work,
                                hipStream_t stream, RenderPending& P) {
    if (!P.pick) return hipSuccess;
    P.pick = false;
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    const int pick = *P.host_pick;
    FrameParams b = P.b;
    if (P.spec_ok && pick > kSpecPick) {
        b.spec = pick - kSpecPick;
        return launch_spec(sc, b, block, d_out, d_work, stream);
    }
    b.walk_team = pick;
    return launch_pass(sc, b, traversal, block, d_out, nullptr, d_work, stream);
}

#endif  // !RT_ACCUM_TU

#if defined(RT_ACCUM_TU) && RT_ACCUM_TU == 1
// One add of a progressive accumulation: the ACC instantiation of the one-pass kernel launch_pass picks
hipError_t launch_accum(const DevScene& sc, const FrameParams& f0, float4* state, int base, int traversal, int block,
                        float* d_out, unsigned int* d_work, hipStream_t stream) {
    if (!state || base < 0 || f0.spp <= base || f0.pass != 0 || f0.pilot != 0) return hipErrorInvalidValue;
    FrameParams fp = f0;
    fp.pilot_state = state;
    fp.pilot = base;
    const KernelKey k = choose_kernel(sc, fp, traversal, false, false, kAccAdd, block);
    return launch_pick(sc, fp, k, block, d_out, nullptr, d_work, stream);
}

#endif  // RT_ACCUM_TU == 1

// rt_adaptive.hip compiles this file a third time (RT_ACCUM_TU 2): the kAccListed instantiations and the
// selection's kernels, in a module of their own for the reason above -- the adds' code object stays what it was
#if defined(RT_ACCUM_TU) && RT_ACCUM_TU == 2
// A listed add (rt_accum_add_selected): f0.spp more samples of each of the *count pixels of list, every pixel
// from the count its state holds.  One pass, one lane per pixel unless teams are set; no sample slices.
hipError_t launch_accum_listed(const DevScene& sc, const FrameParams& f0, float4* state, const uint32_t* list,
                               const uint32_t* count, int traversal, int block, float* d_out, unsigned int* d_work,
                               hipStream_t stream) {
    if (!state || !list || !count || f0.spp < 1 || f0.pass != 0 || f0.pilot != 0) return hipErrorInvalidValue;
    FrameParams fp = f0;
    fp.pilot_state = state;
    fp.pilot_order = list;
    fp.pilot_cost = const_cast<uint32_t*>(count);   // (read only: rt_internal.h)
    fp.slices = 0;
    fp.slice_state = nullptr;
    fp.slice_ready = nullptr;
    const KernelKey k = choose_kernel(sc, fp, traversal, false, false, kAccListed, block);
    return launch_pick(sc, fp, k, block, d_out, nullptr, d_work, stream);
}

// ---- adaptive sampling (rt_accum_mark / rt_accum_select*): which pixels a listed add refines ----
namespace {
constexpr int kSelBlock = 256;

// tile pixel p is a pixel of the frame (not padding of a partial last row)
__device__ __forceinline__ bool tile_pixel_real(int64_t p, int W, int row0, int row_step, int64_t npix) {
    const int64_t krow = p / W;
    return ((int64_t)row0 + krow * row_step) * W + (p - krow * W) < npix;
}

// clamp(acc / s), the operations of accum_resolve_kernel
__device__ __forceinline__ rtm_f3 accum_colour(float4 a, int s) {
    const rtm_f3 o = rtm_div(rtm_v3(a.x, a.y, a.z), (float)s);
    return rtm_v3(rtm_fmax(rtm_fmin(o.x, 1.0f), 0.0f), rtm_fmax(rtm_fmin(o.y, 1.0f), 0.0f),
                  rtm_fmax(rtm_fmin(o.z, 1.0f), 0.0f));
}

// rt_accum_mark: (acc.xyz, s) of every tile pixel
__global__ void accum_mark_kernel(const float4* __restrict__ state, float4* __restrict__ mark, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float4 a = state[2 * p];
    mark[p] = make_float4(a.x, a.y, a.z, state[2 * p + 1].w);
}

// rt_accum_select: flag[p] = the pixel got samples since the mark and its error (rt_api.h) is above the threshold
__global__ void select_error_kernel(const float4* __restrict__ state, const float4* __restrict__ mark,
                                    uint8_t* __restrict__ flag, int64_t n, int W, int row0, int row_step, int64_t npix,
                                    float threshold) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    bool sel = false;
    if (tile_pixel_real(p, W, row0, row_step, npix)) {
        const float4 a = state[2 * p], m = mark[p];
        const int s1 = __float_as_int(state[2 * p + 1].w), s0 = __float_as_int(m.w);
        const rtm_f3 c1 = accum_colour(a, s1), c0 = accum_colour(m, s0);
        const float d = (rtm_fabs(c1.x - c0.x) + rtm_fabs(c1.y - c0.y)) + rtm_fabs(c1.z - c0.z);
        const float e = d / dev_sqrt(((c1.x + c1.y) + c1.z) + 0.01f);
        sel = s1 > s0 && e > threshold;   // (a NaN error compares false)
    }
    flag[p] = sel ? 1 : 0;
}

// rt_accum_select_mask / rt_accum_select_all: flag[p] = src[p] != 0 (src NULL: every pixel), padding pixels 0
__global__ void select_mask_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ flag, int64_t n, int W,
                                   int row0, int row_step, int64_t npix) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    flag[p] = (tile_pixel_real(p, W, row0, row_step, npix) && (!src || src[p] != 0)) ? 1 : 0;
}

// The ordered compaction, three launches: each block of kSelBlock pixels counts its flags; one block turns the
// counts into exclusive offsets and stores their total (the list's length); each block then writes its flagged
// pixels at its offset, in pixel order (a ballot per wave, the waves' totals through LDS).  So list is ascending
// and the same on every run.
__global__ void __launch_bounds__(kSelBlock) select_count_kernel(const uint8_t* __restrict__ flag, int64_t n,
                                                                 uint32_t* __restrict__ block_count) {
    __shared__ unsigned wtot[kSelBlock / 64];
    const int64_t p = (int64_t)blockIdx.x * kSelBlock + threadIdx.x;
    const bool sel = p < n && flag[p] != 0;
    const unsigned long long b = __ballot(sel);
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = (unsigned)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < kSelBlock / 64; ++w) t += wtot[w];
        block_count[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kSelBlock) select_scan_kernel(uint32_t* __restrict__ block_count, int64_t nblocks,
                                                                uint32_t* __restrict__ total) {
    __shared__ unsigned tsum[kSelBlock];
    const int64_t per = (nblocks + kSelBlock - 1) / kSelBlock;
    const int64_t lo0 = (int64_t)threadIdx.x * per, lo = lo0 < nblocks ? lo0 : nblocks;
    const int64_t hi = lo + per < nblocks ? lo + per : nblocks;
    unsigned t = 0;
    for (int64_t q = lo; q < hi; ++q) t += block_count[q];
    tsum[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned run = 0;
        for (int q = 0; q < kSelBlock; ++q) {
            const unsigned v = tsum[q];
            tsum[q] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    unsigned run = tsum[threadIdx.x];
    for (int64_t q = lo; q < hi; ++q) {
        const unsigned v = block_count[q];
        block_count[q] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(kSelBlock) select_compact_kernel(const uint8_t* __restrict__ flag, int64_t n,
                                                                   const uint32_t* __restrict__ block_offset,
                                                                   uint32_t* __restrict__ list) {
    __shared__ unsigned wtot[kSelBlock / 64];
    const int64_t p = (int64_t)blockIdx.x * kSelBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool sel = p < n && flag[p] != 0;
    const unsigned long long b = __ballot(sel);
    if (lane == 0) wtot[wave] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned off = block_offset[blockIdx.x];
    for (int w = 0; w < wave; ++w) off += wtot[w];
    // off + rank < the total of all flags <= n: within list's n entries
    if (sel) list[off + (unsigned)__popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)p;
}

// every tile pixel in order (a full add of an accumulation whose counts differ runs the listed kernel over it)
__global__ void list_all_kernel(uint32_t* __restrict__ list, int64_t n, uint32_t* __restrict__ total) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) list[p] = (uint32_t)p;
    if (p == 0) *total = (uint32_t)n;
}

// s of every tile pixel (rt_accum_sample_map)
__global__ void sample_map_kernel(const float4* __restrict__ state, int32_t* __restrict__ out, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) out[p] = __float_as_int(state[2 * p + 1].w);
}

inline unsigned sel_grid(int64_t n) { return (unsigned)((n + kSelBlock - 1) / kSelBlock); }
}  // namespace

size_t select_scratch_words(int64_t n) { return (size_t)sel_grid(n) + 1; }

hipError_t launch_accum_mark(const float4* state, float4* mark, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(accum_mark_kernel, dim3(sel_grid(n)), dim3(kSelBlock), 0, stream, state, mark, n);
    return hipGetLastError();
}

hipError_t launch_select_error(const float4* state, const float4* mark, uint8_t* flag, const FrameParams& fp,
                               float threshold, hipStream_t stream) {
    if (fp.nloc <= 0) return hipSuccess;
    hipLaunchKernelGGL(select_error_kernel, dim3(sel_grid(fp.nloc)), dim3(kSelBlock), 0, stream, state, mark, flag,
                       fp.nloc, fp.width, fp.row0, fp.row_step, fp.npix, threshold);
    return hipGetLastError();
}

hipError_t launch_select_mask(const uint8_t* src, uint8_t* flag, const FrameParams& fp, hipStream_t stream) {
    if (fp.nloc <= 0) return hipSuccess;
    hipLaunchKernelGGL(select_mask_kernel, dim3(sel_grid(fp.nloc)), dim3(kSelBlock), 0, stream, src, flag, fp.nloc,
                       fp.width, fp.row0, fp.row_step, fp.npix);
    return hipGetLastError();
}

hipError_t launch_select_compact(const uint8_t* flag, int64_t n, uint32_t* scratch, uint32_t* list, uint32_t* count,
                                 hipStream_t stream) {
    if (n <= 0) return hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    const unsigned nb = sel_grid(n);
    hipLaunchKernelGGL(select_count_kernel, dim3(nb), dim3(kSelBlock), 0, stream, flag, n, scratch);
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kSelBlock), 0, stream, scratch, (int64_t)nb, count);
    hipLaunchKernelGGL(select_compact_kernel, dim3(nb), dim3(kSelBlock), 0, stream, flag, n,
                       (const uint32_t*)scratch, list);
    return hipGetLastError();
}

hipError_t launch_list_all(uint32_t* list, int64_t n, uint32_t* count, hipStream_t stream) {
    if (n <= 0) return hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    hipLaunchKernelGGL(list_all_kernel, dim3(sel_grid(n)), dim3(kSelBlock), 0, stream, list, n, count);
    return hipGetLastError();
}

hipError_t launch_sample_map(const float4* state, int32_t* out, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(sample_map_kernel, dim3(sel_grid(n)), dim3(kSelBlock), 0, stream, state, out, n);
    return hipGetLastError();
}

#endif  // RT_ACCUM_TU == 2

#ifndef RT_ACCUM_TU
// rt_accum_read: the frame of an accumulation state, clamp(acc / s) as store_pixel writes it
__global__ void accum_resolve_kernel(const float4* __restrict__ state, float* __restrict__ out, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float4 a = state[2 * p], b = state[2 * p + 1];
    const rtm_f3 o = rtm_div(rtm_v3(a.x, a.y, a.z), (float)__float_as_int(b.w));
    out[3 * p + 0] = rtm_fmax(rtm_fmin(o.x, 1.0f), 0.0f);
    out[3 * p + 1] = rtm_fmax(rtm_fmin(o.y, 1.0f), 0.0f);
    out[3 * p + 2] = rtm_fmax(rtm_fmin(o.z, 1.0f), 0.0f);
}

hipError_t launch_accum_resolve(const float4* state, float* d_out, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(accum_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, state, d_out, n);
    return hipGetLastError();
}

hipError_t launch_rgb8(const float* d_in, uint8_t* d_out, int64_t n, bool gamma, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    // float4 loads and 32-bit stores need 16- and 4-byte alignment (torch / hipMalloc buffers have it)
    if (((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3)) return hipErrorInvalidValue;
    const int block = 256;
    const int64_t grid = ((n + 3) / 4 + block - 1) / block;
    if (gamma)
        hipLaunchKernelGGL(rgb8_kernel<true>, dim3((unsigned)grid), dim3(block), 0, stream, d_in, d_out, n);
    else
        hipLaunchKernelGGL(rgb8_kernel<false>, dim3((unsigned)grid), dim3(block), 0, stream, d_in, d_out, n);
    return hipGetLastError();
}

hipError_t launch_gamma(const float* d_in, float* d_out, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int block = 256;
    const int64_t grid = (n + block - 1) / block;
    hipLaunchKernelGGL(gamma_kernel, dim3((unsigned)grid), dim3(block), 0, stream, d_in, d_out, n);
    return hipGetLastError();
}

#endif  // !RT_ACCUM_TU

}  // namespace rt
