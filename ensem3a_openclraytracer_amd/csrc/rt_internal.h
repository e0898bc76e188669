// Internal interface between the C-ABI layer (rt_api.hip) and the kernels
// (rt_kernels.hip).  Not part of the public boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

#include "rt_layout.h"
#include "rt_slices.h"

namespace rt {

// Device view of one uploaded scene (all pointers are device pointers).
// bits of DevScene::host_flags
constexpr int32_t kHostClusterAuto = 1;   // option "brute_cluster" is -1: only tiles of at least a pixel per resident lane are clustered
constexpr int32_t kHostDirect = 4;        // ... and the enable of the in-place test (option "brute_direct"; rt_debug_last_direct)
constexpr int32_t kHostQuad = 2;          // the shell's record has split faces (option "brute_quad"; rt_debug_last_launch)
constexpr int32_t kHostLean = 8;          // every material emissive or diffuse (HostScene::diffuse_only) and option "brute_lean" not 0
constexpr int32_t kHostPrimary = 16;      // option "brute_primary" not 0: a lean sliced launch traces its camera rays in a pre-pass
struct DevScene {
    // FAST traversal: BVH2 nodes holding both child boxes, 4 x float4 each:
    //   [0] = c0.min.x, c0.max.x, c0.min.y, c0.max.y
    //   [1] = c1.min.x, c1.max.x, c1.min.y, c1.max.y
    //   [2] = c0.min.z, c0.max.z, c1.min.z, c1.max.z
    //   [3] = child refs (int bits): >= 0 internal node, < 0 leaf = ~(48 * triangle), its tri_geo byte offset
    const float4* nodes;
    int32_t nnodes;        // internal nodes in `nodes`
    int32_t root_ref;      // ref of the root (~(48 * tri) when the root is a leaf)
    // the same tree collapsed to 4-wide nodes with quantised child boxes (rt_api.hip emit_wide):
    // 64 bytes per node, 64-byte leaf records (exact leaf box + a.p, e1, e2 + index) in reference
    // DFS rank order; refs >= 0 node, < 0 ~(64 * rank), INT_MIN empty slot
    const float4* wnodes;
    const float4* wleaves;
    int32_t wroot_ref;
    // every quantised child bound with q > 0 lies 2^-17 P outside its exact bound (rt_api.hip emit_wide),
    // which makes the origin-folded dequantisation conservative for ray origins with |o| <= wdq_omax
    // (about 20 P; 0: no gap, exact form only); choose_kernel checks the camera against it per frame
    float wdq_omax;
    float root_box[6];     // min.xyz, max.xyz of the root
    // REF traversal: the reference's own AoS export, 9 floats per node
    const float* bvh9;
    int32_t nbvh9;
    // REF traversal stack capacity: 20 = the reference's (stack.cl:4; a push onto a full stack is dropped,
    // stack.cl:23-24); up to 64 (option "ref_stack") renders the reference's DFS without drops, which
    // separates the pixels a drop changes from those the FAST slab rounding changes
    int32_t ref_stack;
    // triangles in reference order: 3 x float4 (a.p | rank, e1 | index, e2 | 0); REF traversal
    const float4* tri_geo;
    // the same records in the order the FAST tree's leaves are met depth-first (the FAST leaf refs
    // are byte offsets into this array; e1.w gives the triangle's reference index)
    const float4* tri_fast;
    // hit record per triangle: first-vertex normal | material index bits
    const float4* tri_shade;
    // hemisphere frame per triangle (prep_frames_kernel): q, qinv, normalize(n) | colinear flag
    const float4* tri_frame;
    int32_t ntri;
    // materials: the reference's 6 floats [type, r, g, b, roughness, ior] padded to kMatF = 8 (two float4)
    const float* mat;
    int32_t nmat;
    uint32_t near_mask_hi;   // (see near_mask_lo)
    // IBL: the 2x2 texel sums the reference's lookup averages (ibl_sum_kernel), one word per clamped
    // integer coordinate (X, Y) in [0, ibl_w] x [0, ibl_h]: r | g << 10 | b << 20 (each <= 4 x 255)
    const uint32_t* ibl_sum;
    int32_t ibl_w, ibl_h;
    int32_t depth;         // max number of FAST stack entries a ray can need
    // FAST traversal stack: the first stack_lds entries of each lane in LDS, deeper ones
    // (rare) in stack_ovf, a device buffer of (depth - stack_lds) x resident lanes int2 entries
    int32_t stack_lds;
    int2* stack_ovf;
    // FAST on small scenes: one 64-byte record per reachable triangle in reference DFS order
    // (leaf box, a.p, e1, e2, triangle index); nbrute = 0 when the BVH path is used
    const float4* brute;
    int32_t nbrute;
    // option "brute_near" for the instrumented kernels, which walk brute_box and no shell: bit g set (box g < 32 in
    // near_mask_lo, 32 <= g < 64 in near_mask_hi above; boxes past 63 never) = box g is a face of the shell and
    // near_floor is not 0, so rt_count_work* counts the triangle tests the product kernel queues.  (The three
    // "brute_near" fields stand where the structure had padding, behind nbrute, nbox and nmat: no other field
    // moves, and no kernel's arguments do.)
    uint32_t near_mask_lo;
    // the distinct leaf boxes, 2 float4 each (lo.x hi.x lo.y hi.y | lo.z hi.z q0 q1): q0 (and q1 >= 0,
    // int bits) are the records whose leaf box it is.  Padded to whole groups of kBoxGroup (the lock-step
    // loop loads a group with one scalar wait) with a point at 1e30 that lists record 0 alone: a ray
    // with a NaN component, or one from 1e30 (1, 1, 1), passes it (the slab test drops NaN), and then
    // tests record 0 again, which changes no hit.  Every slot's q0 is a valid record and q1 is one or -1
    // (scene_pack.cpp pad_box; tests/test_malformed_inputs.py checks every slot)
    const float4* brute_box;
    int32_t nbox;
    // the lower clamp of the shell's face tests (option "brute_near"): rt::kNearFloor where the
    // packer found every face near-safe (HostScene::shell_floor) and the option is not 0, else 0.0f -- box_hit()'s
    // own clamp
    float near_floor;
    // the same boxes clustered (scene_pack.cpp build_clusters, option "brute_cluster"; ncluster = 0: not
    // clustered): brute_cbox = ncslot slots of brute_box's form, the single boxes padded to nsingle4 (whole
    // groups of kBoxGroup), then kClusterSlots slots per cluster (padded; every padding slot lists record 0
    // alone); brute_crow = 2 float4 per cluster: the union box lo.x hi.x lo.y hi.y | lo.z hi.z, first slot,
    // box count (int bits).  The one-lane product kernels test a cluster's boxes only for the rays that pass
    // its union (rt_device.h trace_brute_compact); the instrumented and team kernels read brute_box.
    const float4* brute_cbox;
    const float4* brute_crow;
    int32_t ncluster, ncslot, nsingle4;
    // host-side flags (launch_pick and its note; no kernel reads them): kHostClusterAuto, kHostQuad below.  One word
    // where the structure had the "brute_cluster is auto" flag, so no kernel's arguments move
    int32_t host_flags;
    // the real single slots at the head of brute_cbox.  The clustered loop tests slots [0, nsingle) and, where a
    // cluster runs lock-step, its `count` boxes in whole groups of kBoxGroup and then the last 1..3 alone: the
    // padding slots stay in memory -- a group load never leaves the buffer, an item's slot index is a shift and
    // a mask -- but only an item tests one
    int32_t nsingle;
    // the shell (scene_pack.cpp build_shell, option "brute_shell"): where its record starts in brute_cbox, in
    // float4 (behind the ncslot slots: 5 float4, then the slots of the singles that are no face); 0: no shell, the
    // clustered loop tests the single slots [0, nsingle).  (It stands where the structure had padding: no other
    // field moves, and no kernel's arguments do.)
    int32_t shell;
};

struct FrameParams {
    float cam[10];
    float env[5];
    int32_t width;       // (int)cam[6]
    int64_t npix;        // frame pixel count (reference imgSize)
    int32_t spp;
    int32_t max_bounce;
    int32_t row0, row_step;
    int64_t nloc;        // pixels in this tile = rows * width
    int32_t resume_min;  // FAST tree walk: resumable traversal, shade once this many lanes are free (0 = off)
    int32_t team;        // brute-force path: lanes per pixel (1, 2, 4, 8; 0 = chosen at launch from the tile size)
    int32_t walk_team;   // FAST tree walk (BVH2 item steps): lanes per pixel walking each ray together (1, 2, 4, 8; 0 = auto)
    int32_t max_waves;   // persistent grid: at most this many waves per SIMD (0 = as many as stay resident)
    int32_t handout;     // pixel hand-out: 0 = chunks interleaved over the XCD groups, 1 = a contiguous block per group
    int32_t step;        // FAST tree walk: 1 = one item per traversal step, 2 = descend-until-leaf rounds, 0 = auto
    // FAST: skip the shadow ray when its result cannot change the sample: envData[3] (sun power) == 0,
    // envData[4] >= 0 and every material colour finite make the sun term of Raytracing.cl:125-137
    // exactly zero whatever the ray hits (set by the host, never for debug logs)
    int32_t sun_skip;
    // FAST tree walk: with no glass material the sun term depends only on whether the shadow ray hits
    // anything (Raytracing.cl:125-137), so its traversal ends at the first accepted triangle
    int32_t sun_any;
    int32_t wide;        // FAST tree walk over the 4-wide quantised layout (DevScene::wnodes)
    int32_t wdq;         // ... with origin-folded dequantisation when DevScene::wdq_omax covers the camera (1, default)
    // a sample that draws no random number (it ends at its first loop head: camera ray escaped or
    // on an emitter) is every later sample of its pixel: the rest are summed without re-running it
    int32_t fixed_point;
    // the shadow ray of a sample's first diffuse or glossy bounce leaves from the same point towards
    // the same sun in every sample of the pixel: traced once, its hit kept (implies fixed_point)
    int32_t sun_cache;
    // Two-pass launches (launch_render, option "pilot"): pass 1 renders the first `pilot` samples of
    // every pixel and saves each unfinished pixel's state (pilot_state: acc.xyz | kc, seed0 seed1 tc s)
    // and the rays it traced (pilot_cost); the pixels are then ordered by that cost, most first
    // (pilot_order); pass 2 continues them in that order, so the last pixels a frame starts are the
    // short ones.  pass 0 = one pass.
    int32_t pass;
    int32_t pilot;
    int32_t pilot_chunk;   // pixels ordered together (consecutive tile pixels; 1 = single pixels)
    int32_t pilot_levels;  // cost bins of the order (2..256); within a bin the chunks keep tile order
    float4* pilot_state;
    uint32_t* pilot_cost;
    uint32_t* pilot_draws;   // BVH2 walk: random numbers each pixel drew in pass 1 (its RNG offset at pilot_state)
    // Pass 2 with sample-parallel speculation (rt_spec.hip, option "spec"): spec trails per pixel, each
    // trail's log of (RNG offset, sample colour) records, spec_cap records per trail; one log per resident
    // lane (a team's trails log the pixel it holds; the logs are reused from record 0 for its next pixel)
    int32_t spec;
    // One-lane brute-force kernels (render_kernel; option "brute_refill", rule below: brute_refill_launch): a
    // wave hands out jobs only once this many of its lanes are free -- or none of its lanes traces, or its
    // hand-out is near its end -- so the hand-out's code, which the whole wave steps through, runs for
    // several lanes at a time.  0 or 1: every lane is refilled at once.  (It stands where the structure had
    // padding: no other field moves, and no kernel's arguments do.)
    int32_t refill;
    float4* spec_log;
    int32_t spec_cap;
    // Sample slices (option "slices", one-pass launches of the tree walk): each pixel's samples are
    // `slices` jobs of spp / slices samples, handed out slice-major (take_pixel), so a lane's last job
    // is a slice, not a whole pixel: the frame's tail shrinks by that factor.  A job that ends a slice
    // stores the pixel's state (slice_state: acc.xyz | kc, seed0 seed1 tc s; write-through) and then the
    // samples done (slice_ready); the job of the next slice, on any lane, waits for that count and
    // continues from the state.  Every pixel's samples run in order: the frame is the one-pass frame.
    // Brute-force scenes (the one-lane kernels, one-pass launches; the three forms of this word are made in one
    // place, rt_slices.h brute_slice_offer / brute_slice_launch): rt_api.hip hands K on, or -K for K on auto;
    // launch_pick decides from its kernel's resident lanes and gives the kernel K | tail << 8 -- only the last
    // tail / 256 of the tile's pixels are sliced, the others are whole jobs handed out first (take_job) -- and
    // the state is 48 bytes per pixel (+ the camera ray's direction; tc shares its word with the cached
    // shadow-ray hit).
    int32_t slices;
    float4* slice_state;
    uint32_t* slice_ready;
    const uint32_t* pilot_order;
    // debug event log of one pixel (rt_debug_pixel_log only; unused by the product launches)
    int64_t log_pixel;
    float* log_buf;
    int32_t log_cap;
    int32_t* log_count;
};
// Progressive accumulation (rt_accum_*): an add runs the ACC instantiations of the render kernels, which are
// always one pass (pass = 0) and read two of the pilot fields in a meaning of their own, so that FrameParams --
// and with it the kernel arguments and the code of the one-shot kernels -- is what it was without them:
//   pilot        the samples earlier adds have done (the launch runs samples pilot .. spp - 1 of every pixel);
//   pilot_state  the accumulation's state buffer (the context's, one per device slot; never d.pilot), in the
//                pilot's layout: two float4 per tile pixel, acc.xyz | kc, seed0 seed1 tc s.
// A pixel's lane restores from it (pilot > 0) and, after sample spp - 1, saves back; out receives
// clamp(acc / spp).  tc is the reference triangle index and kc the hit distance every engine computes alike,
// so any engine continues any other's state.

// A two-pass launch's second pass, waiting for the first: pass 2 launches the kernel the device picked
// (pilot_team_pick_kernel) from the pixels pass 1 left, so the host reads that pick back first.
// launch_render with a RenderPending stops once the pick's copy into pinned host memory is enqueued;
// launch_render_finish waits for it and launches pass 2 (render_host starts every device before it
// waits for any).  Without one, launch_render waits itself.
struct RenderPending {
    bool pick = false;        // pass 2 still to launch
    int* host_pick = nullptr; // pinned host int (the caller's)
    FrameParams b{};          // pass 2's parameters
    bool spec_ok = false;
};
// The scratch of a two-pass launch over a tile of n pixels (rt_api.hip setup_pilot; rt_debug_pilot_order sizes its
// own by the same rule): state 32 B | cost 4 B | order 4 B per pixel, bin totals + offsets (2 x 256), the chunk
// costs + chunk order (at most one chunk per pixel), the sort's segment histograms (256 per 256 chunks) and each
// pixel's pass-1 RNG offset (4 B, pilot_draws).  launch_pilot_order lays the words behind the order out itself.
struct PilotLayout { size_t need, cost, order, draws; };   // bytes; the state is at 0
inline PilotLayout pilot_layout(size_t n) {
    const size_t need = n * 40 + 2 * 256 * sizeof(uint32_t) + 2 * (n + 1) * sizeof(uint32_t) +
                        (n + 256) * sizeof(uint32_t) + n * sizeof(uint32_t);
    return {need, n * 32, n * 36, need - n * sizeof(uint32_t)};
}
// What launch_render remembers of a launch for rt_debug_last_pilot (host integers only): whether it ran two
// passes and, if so, the tile, the pilot samples, the order's chunk and bins as launch_pilot_order took them, and
// the resident lanes the pick was given (0: no pick ran -- a set "walk_team", a set "spec", the brute-force path)
struct PilotNote {
    int two_pass = 0;
    int64_t nloc = 0;
    int pilot = 0, chunk = 0, levels = 0;
    int64_t lanes = 0;
};
// The pass-2 order of a two-pass launch (rt_debug.h rt_debug_pilot_order states it step by step): order[0 .. n) from
// cost[0 .. n), both on the device; order is followed by the scratch words of pilot_layout (bin totals | offs | chunk
// costs | chunk order | segment histograms).  Enqueued on `stream`; launch_render and rt_debug_pilot_order run this.
hipError_t launch_pilot_order(const uint32_t* cost, int64_t n, int chunk, int levels, int pilot, int max_bounce,
                              uint32_t* order, hipStream_t stream);
// ... and its pick: *left = the non-zero words of cost[0 .. n), *ts = the pass-2 kernel for that many pixels on
// `lanes` resident lanes (1, 2 or 4 lanes per pixel; spec: kSpecPick + T trails where teams would be taken)
hipError_t launch_pilot_pick(const uint32_t* cost, int64_t n, int64_t lanes, int spec, unsigned* left, int* ts,
                             hipStream_t stream);
// Launch the render kernel; counts != nullptr selects the instrumented build
// (device pointer to 5 uint64 accumulators).
// d_work: kWorkBytes of device scratch (layout above; the counters are zeroed by the launch).
// note: what rt_debug_last_pilot reports of this launch (may be NULL)
hipError_t launch_render(const DevScene& sc, const FrameParams& fp, int traversal, int block,
                         float* d_out, unsigned long long* d_counts, unsigned int* d_work, hipStream_t stream,
                         RenderPending* pend = nullptr, PilotNote* note = nullptr);
hipError_t launch_render_finish(const DevScene& sc, int traversal, int block, float* d_out, unsigned int* d_work,
                                hipStream_t stream, RenderPending& pend);
// One add of a progressive accumulation (state, base: see above; fp: a one-pass frame, fp.spp = the samples done
// after the add): one pass of the ACC instantiation of the kernel launch_render would pick for fp (sample
// slices as set in fp; no pilot pass, no trails).
hipError_t launch_accum(const DevScene& sc, const FrameParams& fp, float4* state, int base, int traversal, int block,
                        float* d_out, unsigned int* d_work, hipStream_t stream);
// A listed add (rt_accum_add_selected): the kAccListed instantiations, which read two more pilot fields in a
// meaning of their own -- pilot_order is the list of tile pixels to refine (ascending), pilot_cost points at its
// length, a device word the kernel only reads -- and fp.spp is the samples the add gives each listed pixel, on
// top of the count s its state holds (pilot is 0 and unused).  One pass, no slices; one lane per pixel unless
// fp.team / fp.walk_team are set.  out receives clamp(acc / s) of the listed pixels only.
hipError_t launch_accum_listed(const DevScene& sc, const FrameParams& fp, float4* state, const uint32_t* list,
                               const uint32_t* count, int traversal, int block, float* d_out, unsigned int* d_work,
                               hipStream_t stream);
// Adaptive sampling's selection (rt_accum_mark / rt_accum_select*; kernels in rt_adaptive.hip's translation unit):
//   launch_accum_mark      mark[p] = (acc.xyz, s) of the n pixels of a state;
//   launch_select_error    flag[p] = 1 where the pixel got samples since the mark and its error exceeds the
//                          threshold (rt_api.h), else 0; padding pixels of a partial last row 0;
//   launch_select_mask     flag[p] = src[p] != 0 (src NULL: 1), padding pixels 0; src is tile-packed, on the device;
//   launch_select_compact  list = the flagged tile pixels in ascending order, *count = how many; scratch:
//                          select_scratch_words(n) words;
//   launch_list_all        list = 0 .. n - 1, *count = n;
//   launch_sample_map      out[p] = s of the n pixels of a state.
size_t select_scratch_words(int64_t n);
hipError_t launch_accum_mark(const float4* state, float4* mark, int64_t n, hipStream_t stream);
hipError_t launch_select_error(const float4* state, const float4* mark, uint8_t* flag, const FrameParams& fp,
                               float threshold, hipStream_t stream);
hipError_t launch_select_mask(const uint8_t* src, uint8_t* flag, const FrameParams& fp, hipStream_t stream);
hipError_t launch_select_compact(const uint8_t* flag, int64_t n, uint32_t* scratch, uint32_t* list, uint32_t* count,
                                 hipStream_t stream);
hipError_t launch_list_all(uint32_t* list, int64_t n, uint32_t* count, hipStream_t stream);
hipError_t launch_sample_map(const float4* state, int32_t* out, int64_t n, hipStream_t stream);
// Denoised previews (rt_accum_guides*, rt_denoise_device; kernels in rt_denoise.hip's translation unit):
//   launch_accum_guides  d_guides[3 p ..] = the three guide float4 (rt_api.h) of the fp.nloc tile pixels of a
//                        state; fp carries the camera and the tile (check_frame), lconst is device scratch of
//                        launch_const_bytes() that the launch fills with the frame's launch constants;
//   launch_denoise       the filter of rt_api.h over a frame of npix pixels, rows of `width`: d_rgb, d_guides ->
//                        d_out (which may not overlap them); scratch: denoise_scratch_bytes(npix), 16-byte aligned;
//                        lds: the pass at step 1 stages its tile in LDS (the same bits).
size_t launch_const_bytes();
hipError_t launch_accum_guides(const DevScene& sc, const FrameParams& fp, const float4* state, void* lconst,
                               float4* d_guides, hipStream_t stream);
size_t denoise_scratch_bytes(int64_t npix);
hipError_t launch_denoise(const float* d_rgb, const float4* d_guides, int64_t npix, int width, int passes, int nsq,
                          float sigma_c, float sigma_p, bool lds, float4* scratch, float* d_out,
                          hipStream_t stream);
// Temporal reprojection (rt_reproject_device; the kernel in rt_reproject.hip's translation unit): the previous
// frame and guides gathered into the current view, rt_api.h's definition.  basis: rt_reproject_basis' 16 floats less
// the padding; npix > 0 pixels in rows of `width`; guides 16-byte aligned; the outputs overlap nothing.
struct ReprojectBasis { float m[9]; float pos[3]; float f, cam6; };
struct ReprojectParams { float sigma_p, normal_min, max_history, min_weight; };
hipError_t launch_reproject(const float* d_prev_rgb, const float4* d_prev_guides, const float* d_cur_rgb,
                            const float4* d_cur_guides, int64_t npix, int width, const ReprojectBasis& basis,
                            const ReprojectParams& params, float* d_out_rgb, float4* d_out_guides,
                            hipStream_t stream);
// out[3 p ..] = clamp(acc / s) of the n pixels of an accumulation state (rt_accum_read)
hipError_t launch_accum_resolve(const float4* state, float* d_out, int64_t n, hipStream_t stream);
hipError_t launch_prep_frames(const DevScene& sc, float4* frame, hipStream_t stream);
// the IBL's 2x2 texel-sum table (DevScene::ibl_sum) from the RGBA8 image: (w + 1) x (h + 1) words
hipError_t launch_ibl_sum(const uchar4* rgba, int w, int h, uint32_t* sum, hipStream_t stream);
hipError_t launch_gamma(const float* d_in, float* d_out, int64_t n, hipStream_t stream);
hipError_t launch_rgb8(const float* d_in, uint8_t* d_out, int64_t n, bool gamma, hipStream_t stream);
// Sample-parallel speculation (rt_spec.hip): pass 2 of a pilot launch of the BVH2 walk with fp.spec
// trails per pixel; spec_log_bytes = the size of fp.spec_log it needs on a device of `cus` CUs (one log
// per resident lane, launch_spec keeps the grid within them); at most kSpecTrails trails per pixel;
// the device pick of pass 2 (pilot_team_pick_kernel, read back by launch_render) encodes "T trails" as kSpecPick + T
constexpr int kSpecTrails = 8;
constexpr int kSpecPick = 10;
constexpr int kSpecCapMax = 256;   // records per trail log at most (FrameParams::spec_cap)
// resident lanes per CU of the BVH2 walks (render_resume_kernel, spec_kernel: 4 waves per SIMD)
constexpr int kWalkLanesPerCu = 4 * 4 * 64;
size_t spec_log_bytes(const FrameParams& fp, int cus);
hipError_t launch_spec(const DevScene& sc, const FrameParams& fp, int block, float* d_out, unsigned int* d_work,
                       hipStream_t stream);
// The host's rule for FrameParams::refill (option "brute_refill": -1 auto, 0 or 1 off, R >= 2 set).  launch_pick
// applies it where it knows its kernel's resident lanes; rt_debug_brute_refill evaluates it for
// tests/test_brute_refill_rule.py (no frame depends on it).  Auto: R = kRefillBrute on tiles of at least 1.5
// pixels per resident lane (the boundary of the sample slices, rt_slices.h: below it the waves run half empty
// and a waiting lane is a larger share of the work), off elsewhere -- such a launch runs the kernels without the
// threshold's code (launch_pick).  C2 (r12; ms per frame, the parent 6.45): R = 1 / 4 / 6 / 8 / 16
// 6.48-6.52 / 6.28-6.30 / 6.27-6.29 / 6.28-6.31 / 6.54; rows 0::2 (1.6 pixels per lane) 3.74 -> 3.64
constexpr int kRefillBrute = 4;
constexpr int kRefillMax = 64;
inline int brute_refill_launch(int option, int64_t nloc, int64_t lanes) {
    if (option >= 0) return option >= 2 ? (int)std::min<int64_t>(option, kRefillMax) : 0;
    return brute_auto_slices(nloc, lanes) ? kRefillBrute : 0;
}
// Which instantiation of render_kernel / render_resume_kernel a launch runs, as named fields (rt_kernels.hip:
// choose_kernel makes the scene- and frame-level choice, launch_pick refines it with the tile-level rules and
// looks the kernel up in its translation unit's table).  The fields are the kernels' template arguments.
struct KernelKey {
    int trav;     // TRAV_FAST, TRAV_REF
    int count;    // instrumented (rt_count_work*)
    int log;      // debug event log of one pixel
    int smem;     // tree walk with the scene staged in LDS
    int ovf;      // tree walk whose stack spills to DevScene::stack_ovf
    int resume;   // render_resume_kernel (the resumable tree walk); 0: render_kernel
    int step;     // resumable walk: one item per traversal step (0: descend-until-leaf rounds)
    int wide;     // resumable walk: 0 BVH2, 1 the 4-wide layout, 2 ... with origin-folded dequantisation
    int brute;    // render_kernel's BRUTE_: 0 none, 1 lock-step, 2 teams, 3 clustered, | kBruteSliced | kBruteRefill
    int ts;       // resumable walk: lanes per pixel (1, 2, 4, 8)
    int acc;      // 0 one-shot, kAccAdd, kAccListed
    // render_kernel's BRUTE_ bits above kBruteLean (option "brute_primary"; a field of its own: brute keeps its five
    // bits): 0 the kernels above, 1 a lean sliced loop that starts every job from its pixel's record
    // (kBrutePrimary), 2 the pre-pass that writes those records (kBrutePrepass)
    int primary = 0;
};
inline bool operator==(const KernelKey& a, const KernelKey& b) {
    return a.trav == b.trav && a.count == b.count && a.log == b.log && a.smem == b.smem && a.ovf == b.ovf &&
           a.resume == b.resume && a.step == b.step && a.wide == b.wide && a.brute == b.brute && a.ts == b.ts &&
           a.acc == b.acc && a.primary == b.primary;
}
// The lean form of the one-lane brute-force kernels (render_kernel's BRUTE_ bit kBruteLean; option "brute_lean"): a
// loop without the glossy, glass, IBL and pilot code, for the launches whose frame cannot reach any of it.  A launch
// is lean when the kernel launch_pick ends at is a one-lane brute-force product kernel of a one-shot frame (loop 1 or
// 3: no teams, not instrumented, not logging, no accumulation) and brute_lean_frame holds:
//   host_flags & kHostLean   every material's type is 0 or 1, and the option is not 0;
//   env[4] is +0             the IBL term is then so x 0 x e4, which the lean loop writes as so x 0 -- equal bits for
//                            +0 only, so -0, which sample_ibl_if takes for zero as well, keeps the general kernel;
//   pass 0, pilot 0          one pass (a pilot launch's two passes carry state the lean loop does not restore);
//   spp > 0, max_bounce >= 0 the loop's "no sample" and "no bounce" exits are not compiled in;
//   fixed_point, sun_cache   on, their default: the lean loop has them on at compile time.
constexpr int kBruteLean = 16;
// ... and of a lean sliced launch, the form whose camera rays a pre-pass traces (option "brute_primary", -1 or 1 auto,
// 0 off; kHostPrimary): the pre-pass kernel (kBrutePrepass: render_kernel's staging prologue, then one camera ray per
// tile pixel) writes every pixel's slice record -- slice_publish's layout, zero samples done, the camera hit, the
// ray's direction; "all done" for a padding pixel -- and its samples-done word, and the loop kernel (kBrutePrimary)
// starts every job from its pixel's record: no pixel arithmetic, no camera_dir and no PRIMARY trip in the loop.
// Only the template argument carries the two bits; a key has them in KernelKey::primary
constexpr int kBrutePrimary = 32;
constexpr int kBrutePrepass = 64;
inline bool brute_lean_frame(int32_t host_flags, const FrameParams& fp) {
    uint32_t e4;
    std::memcpy(&e4, &fp.env[4], sizeof e4);
    return (host_flags & kHostLean) != 0 && e4 == 0u && fp.pass == 0 && fp.pilot == 0 && fp.spp > 0 &&
           fp.max_bounce >= 0 && fp.fixed_point != 0 && fp.sun_cache != 0;
}
inline bool brute_lean_kernel(const KernelKey& k, int team) {
    return (k.brute & 3) != 0 && (k.brute & 3) != 2 && team <= 1 && k.trav == 0 && !k.count && !k.log && !k.acc && !k.resume;
}
// The engine of a pass over (sc, fp): REF, brute force, the plain, LDS-staged or overflow tree walk, the
// resumable walk with its step and layout.  Pure: no device call.  brute is 0 or 1 and ts 1 here; the tile
// decides the rest (launch_pick).
KernelKey choose_kernel(const DevScene& sc, const FrameParams& fp, int traversal, bool count, bool log, int acc,
                        int block);
// Blocks of fn (block threads, lds bytes of dynamic LDS) the current device keeps resident, at most max_waves
// waves per SIMD (0: no cap); 0 and *err set when the query fails or fn is null.  Each (device, fn, block, lds)
// is queried once: the host query costs more than a launch.
int64_t resident_blocks(const void* fn, int block, size_t lds, int max_waves, hipError_t* err);
// Ray queries (rt_trace*, rt_api.h; kernels in rt_query.hip's translation unit): n rays (two float4 each: dir.xyz
// origin.x | origin.yz tmax reserved) -> n results (k, tri bits, u, v), enqueued on `stream`.  The engine is the one
// choose_kernel would take for the scene (REF, brute force, the 4-wide or the BVH2 walk), in the plain form (one
// thread per ray, the whole stack in LDS) or the persistent one (a resident grid over the ray stream; counter:
// one device word of the caller's, zeroed by the launch).
struct QueryOptions {
    int engine;       // option "query_engine": 0 auto, 1 plain, 2 persistent
    int grid_cap;     // option "query_grid": at most this many blocks of the persistent form (0: the resident ones)
    int resume_min;   // tree walks: new rays are handed out once this many of 64 lanes are free
    int max_waves;    // option "waves"
    int block;
};
hipError_t launch_query(const DevScene& sc, int traversal, int any, const float4* rays, float4* out, int64_t n,
                        const QueryOptions& q, unsigned int* counter, hipStream_t stream);
// Radiance queries (rt_radiance*, rt_camera_rays*, rt_api.h; kernels in rt_radiance.hip's translation unit): n rays
// (two float4 each: dir.xyz origin.x | origin.yz seed0 seed1) -> n state records (two float4 each: sum.xyz k | seed0
// seed1 tri n, save_state's layout), spp samples of naiveGI each, enqueued on `stream`.  REF, brute force (the global
// records) or trace_fast over the BVH2 nodes with the whole stack in LDS: radiance_fits says whether that stack fits a
// block of 64 lanes.  work: radiance_work_bytes() of device scratch (the hand-out counter, zeroed by the launch, and
// the launch constants, made by it).  launch_camera_rays writes rays first .. first + count - 1 of cam's frame of npix
// pixels, with the seeds a render gives those pixels.
constexpr size_t kRadConstOffset = 256;
struct RadianceOptions {
    float env[5];
    int spp, max_bounce;
    int flags;        // rt_radiance.hip: resume, sun_skip, fixed_point, sun_cache
    int grid_cap;     // option "radiance_grid": at most this many blocks (0: the resident ones)
    int max_waves;    // option "waves"
    int block;
};
size_t radiance_work_bytes();
bool radiance_fits(const DevScene& sc, int traversal, int block);
hipError_t launch_radiance(const DevScene& sc, int traversal, const float4* rays, float4* state, int64_t n,
                           const RadianceOptions& q, void* work, hipStream_t stream);
hipError_t launch_camera_rays(const float cam[10], int64_t npix, int64_t first, int64_t count, float4* rays,
                              void* work, hipStream_t stream);
// the scene as the radiance kernels walk it and the largest block <= `block` whose stack fits (0: none does)
int radiance_fit(const DevScene& sc, int trav, int block, DevScene* out);
// Lens frames (rt_lens_radiance*, rt_lens_rays*, rt_radiance_resolve_device, rt_api.h; kernels in rt_lens.hip's
// translation unit): pixels first .. first + count - 1 of cam's frame of npix pixels, spp samples each down a ray of
// its own (lens_ray of rt_api.h) -> count state records, under launch_radiance's engines, options and work block
// (RadianceOptions::flags as rt_radiance.hip's; fixed_point and sun_cache are dropped unless the lens is degenerate).
// launch_lens_rays writes the rays of samples sample0 .. sample0 + nsamples - 1 of those pixels, [count][nsamples]
// rays of two float4; launch_resolve the clamped means of n records, three floats each.
struct LensOptions {
    float jitter, aperture, focus;
    uint32_t seed;
};
hipError_t launch_lens_radiance(const DevScene& sc, int traversal, const float cam[10], int64_t npix, int64_t first,
                                int64_t count, float4* state, const LensOptions& lens, const RadianceOptions& q,
                                void* work, hipStream_t stream);
hipError_t launch_lens_rays(const float cam[10], int64_t npix, int64_t first, int64_t count, int sample0,
                            int nsamples, const LensOptions& lens, float4* rays, void* work, hipStream_t stream);
hipError_t launch_resolve(const float4* state, int64_t n, float* rgb, hipStream_t stream);
// Lens frames inside an accumulation (rt_accum_begin_lens*): the same loop over the tile-packed state
// of fp's tile (fp: check_frame's camera, frame and rows; q.spp = the samples the add gives each job's pixel, on top
// of the count its record holds -- every add resumes).
//   launch_lens_accum_init  the records the tile's pixels start from: sum 0, n 0, the frame's seeds;
//   launch_lens_accum       list NULL: a job per tile pixel; else the pixels list[0 .. *count) (ascending tile pixels,
//                           *count a device word the kernel only reads, at most fp.nloc) -- launch_accum_listed's
//                           list.  Padding pixels of a partial last row get no job;
//   launch_lens_centre      centre[p] = (k, tri bits) of the first hit of tile pixel p's pixel-centre pinhole ray
//                           (rt_camera_rays' ray, traced as rt_trace traces it), 8 bytes per tile pixel;
//   launch_lens_guides      launch_accum_guides with the first hit read from `centre` in place of the state's words.
// work: radiance_work_bytes(), as above.
hipError_t launch_lens_accum_init(const FrameParams& fp, float4* state, hipStream_t stream);
hipError_t launch_lens_accum(const DevScene& sc, int traversal, const FrameParams& fp, float4* state,
                             const uint32_t* list, const uint32_t* count, const LensOptions& lens,
                             const RadianceOptions& q, void* work, hipStream_t stream);
hipError_t launch_lens_centre(const DevScene& sc, int traversal, const FrameParams& fp, float2* centre, void* work,
                              hipStream_t stream);
hipError_t launch_lens_guides(const DevScene& sc, const FrameParams& fp, const float4* state, const float2* centre,
                              void* work, float4* d_guides, hipStream_t stream);
// test hooks
// The process's last render launch (launch_pick) as its kernel got it: the refined key, FrameParams::team,
// walk_team, slices and refill (0: every lane refilled at once), the grid and the dynamic LDS bytes
struct LaunchNote {
    KernelKey key;
    int team, walk_team, slices, refill;
    int64_t grid;
    size_t lds;
    int shell;   // the kernel walks the scene's shell (the clustered loop, DevScene::shell != 0)
    int near;    // ... with a non-zero floor in its face tests (DevScene::near_floor != 0)
    int quad;    // ... and split faces in its record (option "brute_quad")
    int direct;  // ... and the in-place test of the first record enabled in it (option "brute_direct")
    int primary; // the launch's camera rays were traced by a pre-pass (option "brute_primary"; KernelKey::primary 1)
};
void note_launch(const LaunchNote& n);
LaunchNote last_launch();
hipError_t launch_debug_math(int fn, const float* x, const float* y, float* out, int64_t n, hipStream_t stream);
hipError_t launch_debug_log(const DevScene& sc, const FrameParams& fp, int traversal, float* d_out,
                            unsigned int* d_work, hipStream_t stream);
hipError_t launch_debug_trace(const DevScene& sc, int traversal, const float* rays, float* out, int64_t n,
                              hipStream_t stream);
// rt_debug_fn (rt_debug.h lists the functions and their items; kernels in rt_debug_fn.hip's translation unit):
// floats per input / output item of function fn (0: no such function), the device scratch a launch over n items
// needs (16-byte aligned), and the launch over device arrays
constexpr int kDebugFns = 9;
constexpr int debug_fn_in(int fn) {
    constexpr int w[kDebugFns] = {11, 5, 6, 13, 4, 24, 24, 12, 13};
    return fn >= 0 && fn < kDebugFns ? w[fn] : 0;
}
constexpr int debug_fn_out(int fn) {
    constexpr int w[kDebugFns] = {3, 3, 24, 3, 6, 2, 2, 1, 3};
    return fn >= 0 && fn < kDebugFns ? w[fn] : 0;
}
size_t debug_fn_scratch_bytes(int fn, int64_t n);
hipError_t launch_debug_fn(const DevScene& sc, int fn, const float* in, float* out, int64_t n, void* scratch,
                           hipStream_t stream);
// rt_debug_trace_clustered (rt_debug.h; the kernel in rt_debug_fn.hip's translation unit): the clustered product trace
// over n device rays of rt_debug_trace's layout, 256 lanes per block; info: what the kernel walks (clusters, shell,
// floor, split walls).  hipErrorInvalidValue for a scene that is not clustered or does not fit a block's LDS.
hipError_t launch_debug_trace_clustered(const DevScene& sc, const float* rays, float* out, int64_t n, int32_t info[4],
                                        hipStream_t stream);

}  // namespace rt
