/* rt_debug.h -- test hooks of the native library (not part of the drop-in
 * boundary).  Used by tests/ to check the device numerics and single-ray
 * traversal against the CPU oracle. */
#ifndef RT_DEBUG_H
#define RT_DEBUG_H

#include <stdint.h>
#include "rt_api.h"

/* Scheduling and equivalence knobs of rt_set_option (rt_api.h lists the contract's options).  Each
 * renders the same frame as its automatic value (the GPU tests check that bit for bit); the automatic
 * values are the measured defaults.  -1 / 0 = auto where noted.
 *   "resume_min"   resumable tree walk: shade once this many of 64 lanes are free (-1 auto 36 / 48)
 *   "step"         tree-walk traversal loop: 1 one item per step, 2 descend-until-leaf rounds (0 auto)
 *   "team"         brute force: lanes per pixel 1/2/4/8 (0 auto by tile size)
 *   "brute_cluster"  brute force, one lane per pixel: groups of leaf boxes behind one union test, the passing
 *                  rays' (ray, box) tests compacted (0 off, 1 every SAH subtree of 2..8 boxes, -1 auto by cost)
 *   "brute_shell"  clustered brute force: the single boxes that are faces of one box (a room's walls) are tested
 *                  from its six plane distances, computed once per ray (0 off, 1 from two faces, -1 auto from three)
 *   "brute_near"   clustered brute force with a shell: the faces' tests take kNearFloor (rt_layout.h, just under the
 *                  hit condition's 1e-4) as their lower clamp instead of 0 where the packer found every face
 *                  near-safe, so a ray is not tested against the triangles of the wall it starts on (0 off: clamp
 *                  0, -1 auto; 1 means auto: there is no way to force an unsafe floor)
 *   "brute_quad"   clustered brute force with a shell: a ray that is sure which side of a wall's diagonal it leaves
 *                  through queues that side's triangle alone (kQuadBand, kQuadGraze in rt_layout.h; the packer
 *                  splits a wall only where its error bound allows it); packs the scene again (0 off, -1 auto; 1
 *                  means auto: an unsafe wall cannot be forced)
 *   "brute_direct" clustered brute force with a shell: in the one queue step a lane tests the first record of the
 *                  wall it leaves through itself, with the ray it holds, and only second records go to the pair
 *                  queue; packs the scene again (0 off: every record through the queue, -1 auto; 1 means auto)
 *   "brute_refill" brute force, one lane per pixel: a wave hands out jobs once this many lanes are free, 2..64
 *                  (0 or 1 every free lane at once, -1 auto: 4 on tiles of >= 1.5 pixels per resident lane)
 *   "walk_team"    BVH2 walk: lanes walking each ray of a pixel together 1/2/4/8 (0 auto)
 *   "spec"         pass 2 of a pilot launch: speculative trails per pixel 2/4/8 (0 off, -1 auto)
 *   "slices"       one-pass tree-walk launches: sample slices per pixel 2..16 (0 off, -1 auto)
 *   "pilot"        two-pass launches: pilot samples per pixel (0 one pass, -1 auto);
 *   "pilot_chunk", "pilot_levels"  the pass-2 order's chunk of pixels and cost bins (0 auto)
 *   "handout"      pixel hand-out: 1 a contiguous block per XCD group, 0 interleaved chunks (-1 auto)
 *   "wdq"          4-wide walk: origin-folded dequantisation where the builder's gap covers the camera (1)
 *   "waves"        persistent grid: at most this many waves per SIMD (0 = occupancy limit)
 *   "stack_lds"    FAST stack entries per lane kept in LDS, deeper ones in HBM (0 auto)
 *   "sun_skip", "sun_any", "fixed_point", "sun_cache"  exact shortcuts of the shading loop (1 = on)
 *   "denoise_lds"  the denoise filter's pass at step 1 stages its tile and halo in LDS (0 taps from global
 *                  memory, -1 auto: 1) -- the same frame
 *   "query_engine" ray queries: 1 the plain form (one thread per ray, the whole stack in LDS), 2 the persistent
 *                  form (a resident grid over the ray stream), 0 auto -- the same closest hits bit for bit
 *   "query_grid"   ray queries, persistent form: at most this many blocks (0 auto: the resident ones)
 *   "radiance_grid" radiance queries: at most this many blocks of the persistent grid (0 auto: the resident ones) */

#ifdef __cplusplus
extern "C" {
#endif

/* Evaluate a function of the numerics contract (rtm.h) on device 0 over host
 * arrays: fn 0 sin, 1 cos, 2 tan, 3 asin, 4 acos, 5 atan2(x, y), 6 sqrt,
 * 7 x / y, 8 the FAST walks' Moller-Trumbore reciprocal of x (rt_device.h mt_recip: equal to
 * 1.0f / x for 1e-7 <= |x| <= 2^126 and for infinities and NaN), 9 the kernels' sqrtf, 10 their
 * 1.0f / sqrtf(x) (rt_device.h dev_sqrt / dev_inv_sqrt: the IEEE results for every x), 11 their
 * 1.0f / x (dev_recip, likewise).  y may be NULL for unary functions. */
int rt_debug_math(rt_ctx* ctx, int fn, const float* x, const float* y, float* out, int64_t n);

/* Trace n rays (rays[6*i..] = dir.xyz, origin.xyz) through the uploaded
 * scene with the given traversal on device 0; out[2*i] = k, out[2*i+1] =
 * triangle index (-1 = miss). */
int rt_debug_trace(rt_ctx* ctx, int traversal, const float* rays, float* out, int64_t n);

/* Trace n rays (the layout above; the direction is used as given) through the uploaded scene with the clustered
 * brute-force trace of the one-lane product kernels on device 0 -- the device function those kernels call, not a
 * restatement of it: one ray per lane in blocks of 256, the scene staged in LDS as the render kernel stages it, the
 * last wave partial when n is no multiple of 64.  The options "brute_cluster", "brute_shell", "brute_near",
 * "brute_quad" and "brute_direct" act as on a render launch.  out[2*i] = k (1000 on a miss), out[2*i+1] = the bits of the triangle
 * index (-1 = miss).  info: what the kernel walked, as rt_debug_last_launch reports it for a frame: info[0] =
 * clusters, info[1] = 1 when it walked a shell, info[2] = 1 when that shell's floor was not zero, info[3] = 1 when
 * the shell's record has split walls.  RT_ERR_ARG, with a text in rt_last_error, when the uploaded scene has no
 * clustered array (too many triangles for the brute force, or "brute_cluster" left it unclustered): there is no
 * fall-back to another trace. */
int rt_debug_trace_clustered(rt_ctx* ctx, const float* rays, float* out, int64_t n, int32_t info[4]);

/* Evaluate one of the render kernels' own shading and hit functions (rt_device.h: the functions the kernels
 * call, not restatements of them) once per item on device 0.  in holds n items of the function's input
 * floats, out receives n items of its output floats; words marked "bits" carry a 32-bit integer's bit pattern.
 *   fn                in (floats per item)                        out (floats per item)
 *   RT_FN_CAMERA      cam[10], pixel index bits (11)              camera_dir of make_const's constants (3)
 *   RT_FN_SUN         env[5] (5)                                  make_const's sun vector (3)
 *   RT_FN_HEMI        n.xyz, material type 1 or 2, the two RNG    hemi_cosine, hemi_uniform, hemi_sample(true),
 *                     words bits in the samplers' argument        hemi_sample(false), each dir.xyz, invPdf and the
 *                     order (6)                                   two RNG words after, bits (24); all four on the
 *                                                                 frame prep_frames_kernel computes for a triangle
 *                                                                 of normal n and a material of that type
 *   RT_FN_GGX         colour.rgb, roughness, v, l, n (13)         brdf_ggx (3)
 *   RT_FN_IBL         dir.xyz, power (4)                          sample_ibl, then sample_ibl_if(power), on the
 *                                                                 environment rt_set_env uploaded (6)
 *   RT_FN_MT_REF      a.p | 0, e1 | 0, e2 | 0 (the triangle       mt_test: hit 1 / 0, k (1000 on a miss) (2)
 *   RT_FN_MT_FAST     records' three float4), dir.xyz, origin     mt_core: hit 1 / 0, k as computed (2)
 *                     .xyz, 6 unused (24)
 *   RT_FN_BOX_REF     dir, origin, lo.xyz, hi.xyz (12)            the REF traversal's box test ref_box, 1 / 0 (1)
 *   RT_FN_BOX_FAST    dir, origin, lo.xyz, hi.xyz, cull (13)      box_hit(slab(...), cull) with the inverses
 *                                                                 dev_recip(dir) of the FAST walks: 1 / 0, tmin,
 *                                                                 tmax (3)
 * RT_FN_IBL needs an environment; no function needs a scene. */
enum {
    RT_FN_CAMERA = 0, RT_FN_SUN = 1, RT_FN_HEMI = 2, RT_FN_GGX = 3, RT_FN_IBL = 4, RT_FN_MT_REF = 5,
    RT_FN_MT_FAST = 6, RT_FN_BOX_REF = 7, RT_FN_BOX_FAST = 8, RT_FN_COUNT = 9
};
int rt_debug_fn(rt_ctx* ctx, int fn, const float* in, float* out, int64_t n);

/* Render pixel `pixel` of the frame and record its path events (16 floats
 * each: kind 1 bounce ray / 2 sun ray / 3 sample end, j, o.xyz, d.xyz, k or
 * -1, material, sampleOut.xyz, 0,0,0), up to cap events, on device 0. */
int rt_debug_pixel_log(rt_ctx* ctx, int traversal, const float cam[10], const float env[5], int64_t npix, int spp,
                       int max_bounce, int64_t pixel, float* log, int cap, int* n_events, float out3[3]);

/* rt_count_work's five counters for the whole frame plus two wave-level
 * ones: out[5] = traversal-loop iterations issued by waves (an iteration
 * counts once per wave however many lanes take part), out[6] = render-loop
 * iterations of all waves.  out[0] + out[1] over 64 * out[5] is the SIMD
 * efficiency of the traversal loop.  Resumable tree walk only: out[7] / out[8] =
 * clock cycles the waves spent outside / inside the traversal rounds. */
int rt_debug_wave_counts(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp,
                         int max_bounce, uint64_t out[9]);

/* Scene facts: out[0] = FAST layout available (1/0), out[1] = FAST stack
 * depth, out[2] = internal nodes, out[3] = triangles, out[4] = brute-force
 * records (0: the tree walk renders), out[5] = distinct leaf boxes of the
 * brute-force path, out[6] = the largest camera coordinate magnitude for which
 * the 4-wide walk dequantises origin-folded, in millionths (0: never), out[7] = 0. */
int rt_debug_scene_info(rt_ctx* ctx, int64_t out[8]);

/* Host wall times (ms) of the context's last calls, the parts of SURVEY.md 8(d)'s cold t_render
 * (KernelLauncher.py:33-87 pays all of them on every launch_Raytracing): [0] rt_set_scene's validation
 * and repacking (SAH / 4-wide layouts), [1] its uploads and the per-triangle frame kernel, [2]
 * rt_set_env (IBL upload + texel-sum kernel), [3] the last blocking rt_render / rt_render_rgb8
 * (render + read-back). */
int rt_debug_timings(rt_ctx* ctx, double out[4]);

/* Host-only (no device): the per-axis quantisation of the 4-wide layout (rt_api.hip emit_wide).
 * For up to n = 4 child intervals [lo[c], hi[c]] against the lower corner p, returns the biased
 * exponent byte e (scale 2^(e-127)) and byte bounds with p + qlo[c] * 2^(e-127) <= lo[c] and
 * p + qhi[c] * 2^(e-127) >= hi[c] in fp32 and, for every byte q > 0, at least `gap` outside the
 * interval in exact arithmetic (p + qlo s <= lo - gap, p + qhi s >= hi + gap; gap >= 0), or -1 when
 * no scale up to 2^100 does (non-finite bounds, extents beyond 255 * 2^100): the scene then keeps the
 * BVH2 walk (gap = 0) or quantises without the gap (emit_wide). */
int rt_debug_quantise_axis(float p, const float* lo, const float* hi, int n, float gap, uint8_t* qlo, uint8_t* qhi);

/* Host-only (no device): the brute-force box array rt_set_scene would upload for these arrays (the
 * arrays, layout and statuses of rt_scene_check in rt_scene.h; errors through rt_scene_last_error).
 * info[0] = distinct leaf boxes, info[1] = brute-force records (0: the scene renders through the tree
 * walk and the array is one group of padding slots), info[2] = floats in the array: 8 per slot (lo.x
 * hi.x lo.y hi.y lo.z hi.z, then the int bits of the slot's first record and of its second or -1),
 * padding slots up to a whole group of 4 included.  The first min(cap, info[2]) floats are copied to
 * boxes (boxes may be NULL when cap is 0).  The kernels queue the records of every slot that a ray's
 * slab test passes, padding included, so every slot must list valid records. */
int rt_debug_brute_layout(const float* V_p, int64_t n_vp, const float* V_n, int64_t n_vn, const int32_t* faceData,
                          int64_t n_face, const float* materialData, int64_t n_mat, const float* bvh, int64_t n_bvh,
                          int layout, float* boxes, int64_t cap, int64_t info[3]);

/* Host-only (no device): the clustered form of that array which option "brute_cluster" = cluster (-1 auto,
 * 0 off, 1 force) makes rt_set_scene upload beside it.  info[0] = clusters (0: not clustered, both arrays
 * empty), info[1] = single real slots, info[2] = floats in the slot array: 8 per slot as above -- the single
 * slots padded to a whole group of 4, then 8 slots per cluster, its real boxes first --, info[3] = floats in
 * the row array, 8 per cluster: the union box lo.x hi.x lo.y hi.y lo.z hi.z, then the int bits of the
 * cluster's first slot and of its box count.  Every real slot of rt_debug_brute_layout's array appears
 * once; every padding slot lists record 0 alone. */
int rt_debug_brute_clusters(const float* V_p, int64_t n_vp, const float* V_n, int64_t n_vn, const int32_t* faceData,
                            int64_t n_face, const float* materialData, int64_t n_mat, const float* bvh, int64_t n_bvh,
                            int layout, int cluster, float* slots, int64_t slot_cap, float* rows, int64_t row_cap,
                            int64_t info[4]);

/* Host-only (no device): the shell that option "brute_shell" = shell (-1 auto, 0 off, 1 force) makes rt_set_scene
 * upload for a scene clustered with "brute_cluster" = cluster: a box S and the single slots of
 * rt_debug_brute_clusters' array that are faces of it -- flat on one axis at S's lower or upper bound, S's range
 * on the other two, every equality bitwise.  The kernels of the clustered loop test the faces from S's six plane
 * distances, computed once per ray, and the other singles from a slot array of their own.  info[0] = faces (0: no
 * shell, the array is empty; auto takes a shell from 3 faces, force from the 2 that define one), info[1] = single slots that are no face,
 * info[2] = floats in the array: 76 for the record -- S as lo.x hi.x lo.y hi.y lo.z hi.z, the int bits of info[1]
 * and of info[0] | split faces << 8 (rt_debug_brute_quad), then the int bits of the two records of the faces -x, +x, -y, +y, -z, +z (-1 -1: no such face),
 * then seven rows of 8 (rt_debug_brute_quad; the six faces and "no face") -- then 8 per remaining single, in their order, padded to a whole group of 4 as above. */
int rt_debug_brute_shell(const float* V_p, int64_t n_vp, const float* V_n, int64_t n_vn, const int32_t* faceData,
                         int64_t n_face, const float* materialData, int64_t n_mat, const float* bvh, int64_t n_bvh,
                         int layout, int cluster, int shell, float* rec, int64_t cap, int64_t info[3]);

/* Host-only (no device): which boxes of rt_debug_brute_layout's array are near-safe (option "brute_near": flat on
 * one axis, their records in that plane, well conditioned; a ray that passes such a box closer than kNearFloor
 * cannot hit its records), and the floor the shell of rt_debug_brute_shell(cluster, shell) gets.  info[0] = distinct
 * leaf boxes, info[1] = faces of the shell (0: none); the first min(cap, info[0]) flags (1 / 0) are copied to flags
 * (NULL when cap is 0); *floor = kNearFloor when there is a shell and its every face is near-safe, else 0. */
int rt_debug_brute_near(const float* V_p, int64_t n_vp, const float* V_n, int64_t n_vn, const int32_t* faceData,
                        int64_t n_face, const float* materialData, int64_t n_mat, const float* bvh, int64_t n_bvh,
                        int layout, int cluster, int shell, int32_t* flags, int64_t cap, float* floor, int64_t info[2]);

/* Host-only (no device): the walls option "brute_quad" = quad (-1 auto, 0 off, 1 auto) splits in the shell of
 * rt_debug_brute_shell(cluster, shell), per face position -x +x -y +y -z +z.  flags[f]: bit 0 the face is split,
 * bit 1 its first record lies on the side sigma >= 0 of its line; lines[4 f ..]: A.x A.y A.z gamma of sigma(P) =
 * A . P + gamma (A zero on the face's axis, its first non-zero component positive; all zero when not split);
 * words[3 f ..]: the face's packed records first | second << 16 -- both, the one queued for sigma >= 0, the one for
 * sigma < 0 (-1: no such face; 0xffff for a missing second record); recs[18 f ..]: the face's first and second
 * record as Moller-Trumbore reads them, p0 e1 e2 each (zeros where absent); guard = kQuadBand, kQuadGraze, kQuadDirMax
 * (rt_layout.h); info[0] = faces of the shell, info[1] = split faces. */
int rt_debug_brute_quad(const float* V_p, int64_t n_vp, const float* V_n, int64_t n_vn, const int32_t* faceData,
                        int64_t n_face, const float* materialData, int64_t n_mat, const float* bvh, int64_t n_bvh,
                        int layout, int cluster, int shell, int quad, int32_t flags[6], float lines[24],
                        int32_t words[18], float recs[108], float guard[3], int64_t info[2]);

/* Host-only (no device): option "brute_direct" = direct (-1 auto, 0 off, 1 auto) in the shell of
 * rt_debug_brute_shell(cluster, shell).  info[0] = faces of the shell (0: none), info[1] = 1 when its record carries
 * the option's bit -- exactly when the option is not 0 and there is a shell --, info[2] = the record's count word as
 * the kernels load it: faces | split faces << 8 | the bit << 16 (0 without a shell). */
int rt_debug_brute_direct(const float* V_p, int64_t n_vp, const float* V_n, int64_t n_vn, const int32_t* faceData,
                          int64_t n_face, const float* materialData, int64_t n_mat, const float* bvh, int64_t n_bvh,
                          int layout, int cluster, int shell, int direct, int64_t info[3]);

/* 1 when the kernel of the process's last render launch walked a shell whose record carries that bit, else 0. */
int rt_debug_last_direct(void);

/* The count word of the shell's record as the context's scene was packed and uploaded with its options now -- what
 * a render launch's kernel and rt_debug_trace_clustered's load --, 0 when there is no scene or no shell. */
int rt_debug_shell_word(rt_ctx* ctx);

/* No device call: the rule for sample slices on a brute-force scene (option "slices" = option: -1 auto, 0 off,
 * K) for a launch over a tile of nloc pixels on a device that keeps `lanes` lanes of the kernel resident, which
 * brings every pixel to spp samples; accum_base >= 0: an add of a progressive accumulation that has accum_base of
 * them already (-1: a one-shot frame).  out[0] = 1 when the launch takes slices, out[1] = K, out[2] = the share
 * of the tile's pixels that are sliced, in 1/256 (the last ones handed out; 256 = every pixel), else all 0. */
int rt_debug_brute_slices(int64_t nloc, int64_t lanes, int spp, int option, int accum_base, int32_t out[3]);

/* What the kernel of the process's last render launch got as its slice word: 0 for an unsliced launch, K for the
 * tree walk, K | share << 8 (as above) for a sliced brute-force launch. */
int rt_debug_last_slices(void);

/* The process's last render launch, as its kernel got it.  out[0..10] = the kernel's key: traversal (0 FAST,
 * 1 REF), count (instrumented), log, smem (scene staged in LDS), ovf (stack overflow buffer), resume (the
 * resumable tree walk), step (1 item steps, 0 rounds), wide (0 BVH2, 1 the 4-wide layout, 2 with origin-folded
 * dequantisation), brute (0 none, 1 lock-step, 2 teams, 3 clustered, + 4 sample slices, + 8 refill threshold, + 16
 * the lean form: rt_debug_brute_lean),
 * ts (lanes per pixel of the tree walk), acc (0 one-shot, 1 an add, 2 a listed add); out[11..14] = the brute-force
 * team size, the walk's team size, the slice word (rt_debug_last_slices) and R (rt_debug_last_refill) of its
 * parameters; out[15] = blocks launched, out[16] = bytes of dynamic LDS per block; out[17] = 1 when the kernel
 * walked a shell (option "brute_shell": the clustered loop on a scene that has one), else 0; out[18] = 1 when it
 * walked that shell with a non-zero floor (option "brute_near"), else 0; out[19] = 1 when that shell's record has
 * split walls (option "brute_quad"), else 0; out[20] = 1 when a pre-pass traced the launch's camera rays and its
 * kernel started every job from the record of its pixel (option "brute_primary": -1 or 1 auto, 0 off; the lean
 * sliced launches), else 0 -- a field of its own: the key's brute is the same with the option on and off. */
int rt_debug_last_launch(int32_t out[21]);

/* The pass-2 pixel order of a two-pass launch (option "pilot"), computed on device 0 by the launches a render runs
 * (chunk sums, the segmented counting sort, the expansion to pixels) from the caller's costs; it needs no scene.
 * cost[n]: the rays each tile pixel traced in pass 1; order_out[n]: the tile pixel pass 2 starts q-th.  The order:
 *   1. chunks of `chunk` consecutive tile pixels; nfull = n / chunk of them are whole; the sum of a chunk's costs,
 *      modulo 2^32, is its cost v;
 *   2. top = chunk * pilot * 2 * (max(max_bounce, 0) + 1), the most rays a chunk's pilot samples can trace;
 *      scale = max(1, (levels << 16) / max(top, 1)); bin(v) = min(levels - 1, (v * scale) >> 16), the product in
 *      64 bits;
 *   3. the whole chunks in descending order of their bin, chunks of one bin in ascending chunk index (stable);
 *   4. the pixels of a chunk in tile order; the pixels past nfull * chunk keep their place (nfull = 0: the
 *      identity).
 * tests/pilot_ref.py restates it.  RT_ERR_ARG, before any launch, for n <= 0, chunk < 1 or > 4096, levels outside
 * 2..256, pilot < 1 or > 2^20, max_bounce > 4096 (the ranges of the options and of a frame). */
int rt_debug_pilot_order(rt_ctx* ctx, const uint32_t* cost, int64_t n, int chunk, int levels, int pilot, int max_bounce,
                         uint32_t* order_out);

/* The pass-2 pick of a two-pass launch, computed on device 0 by the two launches a render runs, from the caller's
 * costs and for a device that keeps `lanes` lanes of the one-lane walk resident: out[0] = left, the pixels pass 1
 * left unfinished (cost[p] != 0); out[1] = the pick word:
 *   k = 4 when 4 left <= 2 lanes, 2 when 4 left <= 4 lanes, else 1 (lanes per pixel);
 *   spec 0, or k = 1: the word is k;  spec 1 and k > 1: RT_SPEC_PICK + T trails per pixel, T = 8 when 4 left <=
 *   lanes, else k.
 * RT_ERR_ARG, before any launch, for n <= 0, lanes < 1 or spec outside 0..1. */
enum { RT_SPEC_PICK = 10 };
int rt_debug_pilot_pick(rt_ctx* ctx, const uint32_t* cost, int64_t n, int64_t lanes, int spec, int32_t out[2]);

/* What the last rt_render* / rt_count_work* launch of a single-device context did as a two-pass launch, after that
 * launch has been waited for (a blocking render, or the stream of rt_render_device synchronised): info[0] = 1 (two
 * passes ran), info[1] = the tile's pixels nloc, info[2] = the pilot samples per pixel, info[3], info[4] = the
 * order's chunk and bins, info[5] = the resident lanes the pick was given (0: no pick ran -- "walk_team" or "spec"
 * set, or the brute-force path), info[6] = left, the pixels pass 1 left unfinished (where no pick ran, counted by
 * this call), info[7] = the pick word as rt_debug_pilot_pick gives it (0 where no pick ran).  The first min(cap,
 * nloc) words of the costs pass 1 wrote and of the pass-2 order are copied out of the device's scratch, where they
 * stay until the context's next launch (both may be NULL when cap is 0).  RT_ERR_STATE when that launch ran one
 * pass (then nothing is written), RT_ERR_ARG for a context of several devices.  A progressive add is no such
 * launch and leaves the report as it was. */
int rt_debug_last_pilot(rt_ctx* ctx, int64_t info[8], uint32_t* cost_out, uint32_t* order_out, int64_t cap);

/* No device call: the rule for the refill threshold of the one-lane brute-force kernels (option "brute_refill" =
 * option: -1 auto, 0 or 1 off, R = 2..64) for a launch over a tile of nloc pixels on a device that keeps `lanes`
 * lanes of the kernel resident.  *out = R, the free lanes a wave waits for before it hands out jobs, or 0 when
 * every free lane is refilled at once. */
int rt_debug_brute_refill(int64_t nloc, int64_t lanes, int option, int32_t* out);

/* out[0] = R (as above) as the kernel of the process's last render launch got it; out[1], out[2] = the refill
 * counters of the last instrumented launch (rt_count_work*): the render-loop iterations, per wave, that ran the
 * hand-out block, and the lanes that asked for a job in them (out[1] is counts[15] of rt_count_work_detail). */
int rt_debug_last_refill(int64_t out[3]);

/* No device call: the rule for the lean form of the one-lane brute-force kernels (option "brute_lean" = frame[6]: -1
 * auto, 0 off, 1 auto), a loop without the glossy, glass, IBL and pilot code for the frames that reach none of it.
 * materialData: n_mat floats, 6 per material, the type first; env: envData; frame = spp, maxBounce, the launch's pass
 * (0: one pass) and pilot samples, options "fixed_point" and "sun_cache", the option; kernel = what the launch would
 * otherwise run: the brute-force loop (0 none, 1 lock-step, 2 teams, 3 clustered), lanes per pixel, instrumented,
 * logging, accumulation (0 one-shot, 1 an add, 2 a listed add), traversal (0 FAST, 1 REF).  out[0] = 1 when every
 * material's type is 0 or 1 as the kernels read it (an empty table: 1), out[1] = 1 when the launch runs the lean
 * kernel: out[0], the option not 0, a one-lane brute-force product kernel of a one-shot FAST frame, env[4] = +0 (not
 * -0), one pass without a pilot, spp > 0, maxBounce >= 0, fixed_point and sun_cache on.  rt_debug_last_launch reports
 * such a launch with 16 added to its key's brute. */
int rt_debug_brute_lean(const float* materialData, int64_t n_mat, const float env[5], const int32_t frame[7],
                        const int32_t kernel[6], int32_t out[2]);

/* The state records of the open host accumulation (rt_accum_begin or rt_accum_begin_lens), one per frame pixel in the
 * frame's order: every slot's tile-packed state read back and its rows gathered, as rt_accum_read gathers the frame.
 * Blocking; nothing is rendered and the accumulation is untouched.  RT_ERR_STATE without an open, valid host
 * accumulation.  A pixel that has no sample yet holds what its begin left there: a lens accumulation's initial record
 * (sum 0, n 0, the frame's seeds), undefined words for a plain one. */
int rt_debug_accum_state(rt_ctx* ctx, rt_radiance_state* out /* [npix], frame order */);

#ifdef __cplusplus
}
#endif
#endif /* RT_DEBUG_H */
