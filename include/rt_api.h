/* rt_api.h -- C ABI of the MI355X path-tracing integrator.
 *
 * This is the drop-in boundary for the reference's device path:
 *   KernelLauncher(context, platform, device, queue)      KernelLauncher.py:8-31
 *   KernelLauncher.launch_Raytracing(h_img_out, ...)       KernelLauncher.py:33-87
 *   KernelLauncher.launch_ImgProcessing(h_src, h_out, N)   KernelLauncher.py:90-103
 * which build and enqueue the OpenCL kernels
 *   __kernel Raytracing      Kernels/Raytracing.cl:161-221
 *   __kernel ImgProcessing   Kernels/ImgProcessing.cl:1-10
 * The Python mirror of KernelLauncher (ensem3a_openclraytracer_amd/KernelLauncher.py)
 * binds these entry points with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions: every function returns 0 on success and a non-zero rt_status
 * otherwise; rt_last_error(ctx) (or rt_last_error(NULL) for failures without
 * a context) then describes the failure.  Host pointers are borrowed for the
 * duration of the call only.  Calls on one context are not thread-safe; use
 * one context per host thread.  No torch types cross this boundary.
 */
#ifndef RT_API_H
#define RT_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_ctx rt_ctx;

enum rt_status {
    RT_OK = 0,
    RT_ERR_ARG = 1,       /* invalid argument (shape, index out of range, ...) */
    RT_ERR_HIP = 2,       /* HIP runtime error */
    RT_ERR_STATE = 3,     /* call out of order (e.g. render before set_scene) */
    RT_ERR_SCENE = 4,     /* scene data the kernels cannot accept (bad material type, malformed BVH) */
    RT_ERR_DEGENERATE = 5 /* BVH build would not terminate in the reference (duplicate centroids) */
};

/* Traversal algorithm (rt_set_option "traversal"). */
enum rt_traversal {
    RT_TRAVERSAL_FAST = 0, /* closest-first BVH2 with t-culling and DFS-rank tie break (default) */
    RT_TRAVERSAL_REF = 1   /* the reference's own DFS (MathLib.cl:234-288): no culling, 20-slot stack */
};

/* Tree the FAST traversal walks (rt_set_option "bvh").  Both trees hold the
 * reference's leaf boxes bit for bit and give identical hits; SAH regroups
 * them so fewer nodes are visited. */
enum rt_bvh_layout {
    RT_BVH_REFERENCE = 0, /* the BVH.py tree as exported */
    RT_BVH_SAH = 1        /* surface-area-heuristic regrouping (default) */
};

/* Create a context on n_devices HIP devices (device_ids may be NULL = 0..n-1; explicit ids may
 * repeat a device: each slot renders its own interleaved rows with its own stream and buffers).
 * Replaces the pyopencl Context/CommandQueue/Program build of
 * KernelLauncher.__init__ (KernelLauncher.py:8-31). */
int rt_create(int n_devices, const int* device_ids, rt_ctx** out);
void rt_destroy(rt_ctx* ctx);
/* Last error message of ctx (or of the calling thread when ctx is NULL). */
const char* rt_last_error(rt_ctx* ctx);

/* Upload the scene (replaces the per-launch cl.Buffer uploads of
 * KernelLauncher.py:41-57).  Arrays are the reference's flat layouts:
 * vp/vn float32[3*N], vuv float32[2*N] (may be NULL/empty, never read),
 * face int32[10*T] = [mat, uv0..2, n0..2, p0..2], mat float32[6*M],
 * bvh9 float32[9*nodes] = BVH.py export [L, R, min.xyz, max.xyz, tri|-1].
 * Counts are element counts.  The arrays are copied; the caller may free them. */
int rt_set_scene(rt_ctx* ctx, const float* vp, int64_t nvp, const float* vn, int64_t nvn,
                 const float* vuv, int64_t nvuv, const int32_t* face, int64_t nface,
                 const float* mat, int64_t nmat, const float* bvh9, int64_t nbvh);

/* Upload the IBL environment map: RGBA8, row-major, w*h texels (replaces the
 * cl.Image of KernelLauncher.py:71-72). */
int rt_set_env(rt_ctx* ctx, const uint8_t* rgba, int w, int h);

/* Integer options of the drop-in contract:
 *   "traversal"  an rt_traversal value: FAST (default) or REF = the reference's own DFS, stack.cl's 20 slots;
 *   "bvh"        an rt_bvh_layout value: the tree the FAST walk uses, SAH by default -- same hits;
 *   "bvh_width"  FAST tree walk: 2 = BVH2 nodes, 4 = the 4-wide quantised layout, 0 = auto (4-wide when
 *                the BVH2 node array exceeds 16 MB) -- same frame;
 *   "brute_max"  FAST on scenes of at most this many triangles tests every leaf box in lock-step instead
 *                of walking a tree (default 64, 0 = always walk) -- same hits;
 *   "ref_stack"  REF's stack slots (20 = the reference's; more = no silent drops: the only option that
 *                changes a frame);
 *   "block"      threads per block: 64, 128 or 256.
 * "bvh" and "brute_max" may be changed after rt_set_scene.  Every other key rt_set_option accepts is a
 * scheduling / equivalence knob listed in rt_debug.h: each renders the same frame, and the automatic
 * values are the measured defaults. */
int rt_set_option(rt_ctx* ctx, const char* key, int64_t value);

/* Render one frame, blocking, into caller-owned host memory out_rgb[3*npix]
 * (row-major RGB, clamped to [0,1]).  Semantics of
 * launch_Raytracing(out, ..., cam, envData, imgDim=npix, spp, maxBounce, IBL):
 * the row width is (int)cam[6] and pixel i gets RNG seeds (i % npix, i / npix).
 * With several devices the rows are interleaved over them (row r on device
 * r mod n) and each device copies its rows back. */
int rt_render(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp,
              int max_bounce, float* out_rgb);

/* Asynchronous render of the rows row0, row0+row_step, ... (row width
 * (int)cam[6], frame of npix pixels) on device device_index into DEVICE
 * memory d_out (packed: row k of the tile at d_out[3*W*k]), enqueued on the
 * HIP stream `stream` (a hipStream_t; NULL = the default stream).  Used
 * by the multi-process (one rank per GPU) path and the benchmark.  Returns
 * after the launch is enqueued. */
int rt_render_device(rt_ctx* ctx, int device_index, const float cam[10], const float env[5],
                     int64_t npix, int spp, int max_bounce, int row0, int row_step,
                     float* d_out, void* stream);

/* Number of rows rt_render_device writes for (npix, W, row0, row_step). */
int64_t rt_tile_rows(int64_t npix, int width, int row0, int row_step);

/* Progressive rendering: accumulate the samples of one frame over several calls.  The reference sums a
 * pixel's samples in order over one RNG chain, divides by the count and clamps (Raytracing.cl:191-220), so
 * adds of a and then b samples give, bit for bit, the frame of a one-shot render at a + b samples.
 *
 * A context holds at most one accumulation.  Its per-pixel state (sum, RNG words, the cached camera hit as
 * reference triangle index and distance, samples done: 32 bytes per pixel) lives in a device buffer of its
 * own per device slot: rt_render*, rt_count_work* and the debug entry points may be called between two adds.
 *   rt_accum_begin     open an accumulation of the frame (cam, env, npix, max_bounce as rt_render; the same
 *                      argument checks), no samples yet; replaces an open one.
 *   rt_accum_add       run spp >= 1 more samples of every pixel, blocking; out_rgb[3*npix] (may be NULL)
 *                      receives clamp(sum / total) exactly as rt_render at the total would write it.  Rows
 *                      are split over the device slots as in rt_render.
 *   rt_accum_add_rgb8  the same, the frame quantised on the device(s) as rt_render_rgb8 does (a preview).
 *   rt_accum_read      the frame at the samples done; nothing is rendered.
 *   rt_accum_samples   samples done per pixel; -1 when no accumulation is open (NULL context: -1).
 *   rt_accum_end       free the state (no error when none is open).
 * Limit: the total may not exceed RT_ACCUM_MAX_SAMPLES (2^24: the sample count stays exact as a float
 * divisor and the sample-slice arithmetic of an add within 32 bits); an add past it, or spp < 1, is
 * RT_ERR_ARG and adds nothing.
 * RT_ERR_STATE: add or read with no accumulation open, read before the first add, and add or read after the
 * accumulation was invalidated.  rt_set_scene, rt_set_env and rt_set_option of "traversal" or "ref_stack"
 * invalidate it (rt_accum_samples stays readable; begin again or end it).  Every other option keeps it
 * valid -- "bvh", "brute_max" and "bvh_width" included: they give the same hits, and the state is
 * engine-neutral.  Scheduling: an add is always one pass; it takes sample slices as a one-shot render
 * would, over the samples it adds, and never a pilot pass or speculative trails ("pilot" and "spec" do not
 * apply to it). */
#define RT_ACCUM_MAX_SAMPLES (1 << 24)
int rt_accum_begin(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int max_bounce);
int rt_accum_add(rt_ctx* ctx, int spp, float* out_rgb);
int rt_accum_add_rgb8(rt_ctx* ctx, int spp, int gamma, uint8_t* out_rgb8);
int rt_accum_read(rt_ctx* ctx, float* out_rgb);
int64_t rt_accum_samples(rt_ctx* ctx);
int rt_accum_end(rt_ctx* ctx);
/* Tile form, for the one-rank-per-GPU path: the state is per (context, device slot).
 *   rt_accum_begin_device  open an accumulation of the rows row0, row0 + row_step, ... on slot device_index
 *                          (replaces that slot's; rt_accum_begin is this call on every slot, row k of n).
 *   rt_accum_add_device    enqueue spp more samples of the tile on the HIP stream `stream` (NULL = the
 *                          default stream) into DEVICE memory d_out, packed as rt_render_device packs it.
 * Asynchrony: rt_accum_add_device returns once the launch is enqueued, as rt_render_device does; unlike
 * rt_render_device it never waits on the stream (it has no pilot pass whose result the host reads).  The
 * state and d_out are complete when the work enqueued on `stream` is; adds on different streams are ordered
 * by the context, as its renders are.  rt_accum_samples counts an add from the moment it is enqueued. */
int rt_accum_begin_device(rt_ctx* ctx, int device_index, const float cam[10], const float env[5],
                          int64_t npix, int max_bounce, int row0, int row_step);
int rt_accum_add_device(rt_ctx* ctx, int device_index, int spp, float* d_out, void* stream);

/* Adaptive sampling: add samples only to the pixels that still need them.  The contract stays exact: a pixel
 * that has received n samples holds the value of the one-shot frame at n spp, bit for bit, whatever the other
 * pixels received (the state carries each pixel's own count, and a pixel's samples run in order over its own
 * RNG chain).
 *   rt_accum_mark        snapshot (sum, count) of every pixel: 16 bytes per pixel, in a buffer of its own per
 *                        slot that is allocated on first use.
 *   rt_accum_select      on the device, per pixel: c1 = clamp(sum / count) as rt_accum_read gives it, c0 the
 *                        same from the mark, and in fp32, evaluated in this order without contraction,
 *                            d = (|c1.x - c0.x| + |c1.y - c0.y|) + |c1.z - c0.z|
 *                            n = sqrt(((c1.x + c1.y) + c1.z) + 0.01f)        (correctly rounded)
 *                            e = d / n                                       (correctly rounded)
 *                        The pixel is selected iff it received samples since the mark and e > threshold (a
 *                        NaN error does not select).  The selected pixels are kept as a list in ascending
 *                        pixel order, built by a scan -- the same list on every run; *n_selected (may be
 *                        NULL) receives its length.
 *   rt_accum_select_mask the same list from the caller's mask[npix] (non-zero = selected): a region of
 *                        interest, or a policy of the caller's own.  rt_accum_select_all selects every pixel.
 *   rt_accum_selection   the current selection as a 0/1 mask_out[npix].
 *   rt_accum_sample_map  out[npix] = samples done, pixel by pixel.
 *   rt_accum_add_selected  spp >= 1 more samples of every selected pixel, each continuing from its own count,
 *                        blocking; out_rgb[3*npix] (may be NULL) receives the whole frame, clamp(sum / count) at
 *                        each pixel's own count.  An empty selection adds nothing (RT_OK, the frame as it is).
 *                        The selection stays: it may be added to again.
 * After a selected add the counts differ: rt_accum_samples returns the largest a pixel can hold (the full adds
 * plus every selected add -- the largest count itself when the selections were nested, as rt_accum_select's
 * are), RT_ACCUM_MAX_SAMPLES is checked against it, and rt_accum_add still adds spp samples to every pixel,
 * each from its own count.
 * RT_ERR_STATE: rt_accum_select without a mark; rt_accum_add_selected and rt_accum_selection without a
 * selection; rt_accum_add_selected before the first rt_accum_add (every pixel needs a sample: its cached
 * camera hit); mark, select and sample map before any sample; any of them after an invalidation.  RT_ERR_ARG:
 * spp < 1, or an add past RT_ACCUM_MAX_SAMPLES; nothing is added.  Mark and selection are dropped by begin, by
 * end and by whatever invalidates the accumulation.
 * Scheduling: a selected add is one pass over the list -- no pilot, no trails, no sample slices ("pilot",
 * "spec" and "slices" do not apply) -- with one lane per pixel unless "team" / "walk_team" are set, which are
 * honoured with the same bits. */
int rt_accum_mark(rt_ctx* ctx);
int rt_accum_select(rt_ctx* ctx, float threshold, int64_t* n_selected);
int rt_accum_select_mask(rt_ctx* ctx, const uint8_t* mask);
int rt_accum_select_all(rt_ctx* ctx);
int rt_accum_selection(rt_ctx* ctx, uint8_t* mask_out);
int rt_accum_sample_map(rt_ctx* ctx, int32_t* out);
int rt_accum_add_selected(rt_ctx* ctx, int spp, float* out_rgb);
/* Tile forms: one slot, the HIP stream `stream`, enqueue only, as rt_accum_add_device is -- none of them waits,
 * the list's length stays in device memory, and a select followed by rt_accum_add_selected_device on the same
 * stream needs no host wait in between.  d_mask is DEVICE memory, one byte per tile pixel, packed as the
 * tile's rows are (rt_tile_rows x width); d_out as for rt_accum_add_device, the whole tile. */
int rt_accum_mark_device(rt_ctx* ctx, int device_index, void* stream);
int rt_accum_select_device(rt_ctx* ctx, int device_index, float threshold, void* stream);
int rt_accum_select_mask_device(rt_ctx* ctx, int device_index, const uint8_t* d_mask, void* stream);
int rt_accum_select_all_device(rt_ctx* ctx, int device_index, void* stream);
int rt_accum_add_selected_device(rt_ctx* ctx, int device_index, int spp, float* d_out, void* stream);

/* Denoised previews: first-hit guide buffers out of the accumulation's state, and an edge-aware filter they
 * drive.  Nothing is rendered, no ray is traced and the state is untouched: rt_accum_read before and after
 * gives the same bits.  (One exception to "no ray is traced": the first guides call of a lens accumulation traces
 * the pixel-centre ray of every tile pixel once -- rt_accum_begin_lens, contract E3.)
 *
 * Guides: three float4 per pixel (12 floats), from the pixel's cached camera hit and its own sample count.
 *   G0 = (n.x, n.y, n.z, k)   n the normal the shading uses (the first vertex's, face[4]), k the hit distance;
 *                             a miss gives (0, 0, 0, -1);
 *   G1 = (P.x, P.y, P.z, f)   P = o + d * k per component (one multiply, then one add) on the pixel's camera ray,
 *                             0 on a miss; f (int bits) = the pixel's sample count where it is filterable, else 0;
 *   G2 = (a.r, a.g, a.b, m)   m (int bits) the material index, -1 on a miss; a = max(colour, 0.01f) per channel
 *                             of a filterable pixel, else (1, 1, 1).
 * A pixel is filterable when its first hit's material is of type 1 (diffuse) or 2 (glossy).  Misses and emitters
 * draw no random number and carry no noise; a glass first hit shows geometry the guides do not describe.
 * Apart from f the guides do not depend on the samples added.
 *   rt_accum_guides         host form, out[12 * npix] in frame order;
 *   rt_accum_guides_device  slot device_index's tile into DEVICE memory d_guides, packed as d_out of
 *                           rt_accum_add_device is (12 floats per tile pixel, 16-byte aligned); padding pixels of
 *                           a partial last row get the miss pattern (f = 0, m = -1).  Enqueues on `stream`
 *                           and never waits.
 * RT_ERR_STATE with no accumulation open, before the first add, or after an invalidation; RT_ERR_ARG for a NULL
 * output.
 *
 * The filter (rt_denoise_device) is a whole-frame image operation on one device, independent of the accumulation:
 * d_rgb[3 * npix] and d_guides[12 * npix] in frame order (rows of `width`, H = ceil(npix / width) rows) give
 * d_out[3 * npix], which may not overlap them.  A NULL params means the defaults.  Definition -- everything is
 * fp32, evaluated in the order written, without contraction:
 *   1. Demodulate: a filterable pixel (f > 0) has x = c / a per channel.  Any other pixel is not filtered: its
 *      output is its input, copied bit for bit.
 *   2. Pass i = 0 .. passes - 1, step = 1 << i, for each filterable pixel p: acc = 0, ws = 0; taps dy = -2 .. 2
 *      (outer), dx = -2 .. 2 (inner), q = p + (dx, dy) * step, h = K[|dx|] * K[|dy|], K = {3/8, 1/4, 1/16}.
 *      The centre tap has w = h (9/64).  A tap outside [0, width) x [0, H), one whose pixel index is >= npix,
 *      and a tap on a pixel that is not filterable have w = 0.  Otherwise
 *          t   = max(0, (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z)
 *          wn  = t, squared normal_squarings times
 *          d   = P_q - P_p;  dpl = |(n_p.x * d.x + n_p.y * d.y) + n_p.z * d.z|
 *          a_  = dpl / (sigma_p * k_p);  wp = 1 / (1 + a_ * a_)
 *          dc  = x_q - x_p (this pass's input);  d2 = (dc.r * dc.r + dc.g * dc.g) + dc.b * dc.b
 *          sc2 = ((sigma_c * sigma_c) / (float)s_p) / (float)(step * step);  wc = 1 / (1 + d2 / sc2)
 *          w   = (h * (wn * wp)) * wc
 *      then acc += w * x_q per channel (multiply, then add) and ws += w; after the taps x'_p = acc / ws
 *      (ws >= 9/64).  A pass reads only the previous pass's output.
 *   3. Remodulate: out = max(min(x * a, 1), 0).
 * The colour bandwidth narrows with 1 / sqrt(s_p) as Monte-Carlo noise does, so it follows each pixel's own count.
 * rt_denoise_device enqueues on `stream` and waits only when its scratch buffers (64 bytes per pixel, the device
 * slot's, allocated on first use) have to grow.  RT_ERR_ARG: NULL buffers, npix < 1, width < 1, passes outside
 * 1..8, normal_squarings outside 0..8, a sigma that is not finite and > 0.
 *   rt_accum_denoise  host form: resolves the frame and the guides on every slot, filters the whole frame on slot
 *                     0 (with several slots the rows are assembled there through the host) and reads
 *                     out_rgb[3 * npix] back, blocking.  Errors as rt_accum_read, and RT_ERR_ARG as above. */
typedef struct {
    int passes;              /* 1..8, default 5: step 1, 2, 4, ... */
    int normal_squarings;    /* 0..8, default 5 */
    float sigma_c, sigma_p;  /* > 0, finite; defaults 1.5f, 0.02f */
} rt_denoise_params;
int rt_accum_guides(rt_ctx* ctx, float* out);
int rt_accum_guides_device(rt_ctx* ctx, int device_index, float* d_guides, void* stream);
int rt_denoise_device(rt_ctx* ctx, int device_index, const float* d_rgb, const float* d_guides, int64_t npix,
                      int width, const rt_denoise_params* params, float* d_out, void* stream);
int rt_accum_denoise(rt_ctx* ctx, const rt_denoise_params* params, float* out_rgb);
/* rt_denoise: rt_denoise_device on HOST arrays rgb[3 * npix], guides[12 * npix] -> out_rgb[3 * npix], blocking
 * (slot 0): the filter for a frame that is not the accumulation's own, such as rt_accum_reproject's.  Errors as
 * rt_denoise_device. */
int rt_denoise(rt_ctx* ctx, const float* rgb, const float* guides, int64_t npix, int width,
               const rt_denoise_params* params, float* out_rgb);

/* Temporal reprojection: carry a frame's history across a camera move.  The previous view's frame and guides are
 * gathered into the current view -- G1 is every pixel's world-space first hit, G0 and G2 say whether two pixels see
 * the same surface -- and blended with the current frame by sample counts.  One image-space kernel: no ray is
 * traced and no accumulation state is touched, so rt_accum_read stays the exact frame.  Scene and environment must
 * be what they were when the history was made: that is the caller's job, nothing here can check it.
 *
 * The history length lives in the guides' f word: in prev_guides f > 0 means "filterable, with this many samples'
 * worth of history"; out_guides is cur_guides with f raised to the blended count.  out_guides therefore goes
 * straight into rt_denoise_device, whose colour bandwidth narrows accordingly, and it is the prev_guides of the
 * next move: frames chain without a side buffer.
 *
 * rt_reproject_basis (host only, no GPU call): the previous camera as the 16 floats the kernel takes.
 *   basis[0..8]   M, row-major: column j is the unit vector e_j taken through rtm_rotate about z by
 *                 -(cam[5] * (3.14f / 180.0f)), then about y by -(cam[4] * ...), then about x by -(cam[3] * ...):
 *                 genCameraRay's three rotations (Raytracing.cl:18-37) undone, in reverse order;
 *   basis[9..11]  cam[0..2], the position;
 *   basis[12]     cam[1] - focal.y with focal.y = cam[1] - 1.0f / (2.0f * tan(cam[9] / 2.0f)) as the frame's launch
 *                 constants have it: the focal length f;
 *   basis[13]     cam[6];  basis[14..15] = 0.
 * RT_ERR_ARG: a NULL pointer or a cam that is not finite.
 *
 * Definition, per pixel p < npix -- everything is fp32, evaluated in the order written, without contraction;
 * W = width, H = ceil(npix / W), the guides split as above (n, k | P, f | a, m), min(x, y) = x < y ? x : y:
 *   0. f_p <= 0 (a miss, an emitter, glass): no history.
 *   1. v = P_p - pos;  l.x = (M00 * v.x + M01 * v.y) + M02 * v.z, l.y and l.z likewise from rows 1 and 2.
 *      !(l.y > 0): no history.
 *   2. t = f / l.y;  u = (l.x * t + 0.5f) * cam6;  vv = (0.5f - l.z * t) * cam6 -- the continuous pixelY (column)
 *      and pixelX (row) of genCameraRay.  !(u >= -1 && u < (float)W && vv >= -1 && vv < (float)H): no history
 *      (a NaN fails it).  c0 = floorf(u), r0 = floorf(vv), fu = u - c0, fv = vv - r0.
 *   3. acc = 0, ws = 0, hs = 0.  Four taps (dr, dc) = (0,0), (0,1), (1,0), (1,1) in that order: c = (int)c0 + dc,
 *      r = (int)r0 + dr, b = (dc ? fu : 1 - fu) * (dr ? fv : 1 - fv), and the tap's pixel index is
 *          q = (r + 1) * W + c - 1,
 *      the inverse of genCameraRay's pixelY = (i + 1) % W, pixelX = (i - pixelY) / W, exact for every i >= W - 1
 *      (indices 0 .. W - 2 duplicate row 0 and are never taps).  A tap is valid iff 0 <= c < W, r >= 0, q < npix,
 *      f_q > 0, m_q == m_p, (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z >= normal_min, and with d = P_q - P_p
 *      |(n_p.x * d.x + n_p.y * d.y) + n_p.z * d.z| <= sigma_p * k_p  (n, k, P, f, m of q from prev_guides).
 *      A valid tap adds: acc += b * (prev_rgb_q / a_q) per channel (divide, multiply, then add); ws += b;
 *      hs += b * (float)f_q.
 *   4. !(ws >= min_weight && ws > 0): no history.  Else hx = acc / ws, h = min(hs / ws, max_history).
 *   5. x_p = cur_rgb_p / a_p;  s = (float)f_p;  tot = h + s;  x = (hx * h + x_p * s) / tot per channel;
 *      out_rgb_p = max(min(x * a_p, 1), 0) (rtm.h's fmin, fmax: a NaN goes to 1);  out_guides_p = cur_guides_p
 *      with f = (int)tot, or 2147483647 when !(tot < 2^31).
 *   6. "No history" anywhere above: out_rgb_p and out_guides_p are the current inputs, copied bit for bit.
 * The defaults (a NULL params): sigma_p = 0.02f, the filter's plane tolerance with the same meaning;
 * normal_min = 0.9f; max_history = 64; min_weight = 0.25f.
 *
 *   rt_reproject_device  whole frames in DEVICE memory on slot device_index, independent of the accumulation:
 *                        rgb arrays of 3 * npix floats, guide arrays of 12 * npix floats, 16-byte aligned, in frame
 *                        order.  The outputs may overlap neither an input nor each other; d_prev_* may be d_cur_*.
 *                        The basis is evaluated on the host by rt_reproject_basis and passed to the kernel by value.
 *                        Enqueues on `stream` and never waits.
 *   rt_accum_reproject   host form on the open accumulation, plain or lens: resolves its frame and guides on every
 *                        slot, reprojects the HOST arrays prev_rgb[3 * npix], prev_guides[12 * npix] into it on slot
 *                        0 and reads out_rgb[3 * npix] and out_guides[12 * npix] back, blocking.  The width is the
 *                        accumulation's.  Errors as rt_accum_read; the state is untouched.
 * RT_ERR_ARG: NULL buffers, npix < 1, npix >= 2^31, width < 1, (int)prev_cam[6] != width, a prev_cam that is not
 * finite (or whose basis is not), sigma_p or max_history not finite and > 0, normal_min or min_weight not finite,
 * misaligned guides, outputs that overlap.  Nothing is enqueued and no output is written. */
typedef struct { float sigma_p, normal_min, max_history, min_weight; } rt_reproject_params; /* 16 bytes */
int rt_reproject_basis(const float cam[10], float basis[16]);
int rt_reproject_device(rt_ctx* ctx, int device_index, const float* d_prev_rgb, const float* d_prev_guides,
                        const float prev_cam[10], const float* d_cur_rgb, const float* d_cur_guides, int64_t npix,
                        int width, const rt_reproject_params* params, float* d_out_rgb, float* d_out_guides,
                        void* stream);
int rt_accum_reproject(rt_ctx* ctx, const float* prev_rgb, const float* prev_guides, const float prev_cam[10],
                       const rt_reproject_params* params, float* out_rgb, float* out_guides);

/* Ray queries: closest-hit and any-hit batches of the caller's own rays through the uploaded scene (no
 * counterpart in the reference).  Picking off the pixel grid, visibility between two points, ambient-occlusion or
 * light-map baking, an integrator of the caller's own: the hits are the frame's hits, bit for bit.
 *
 * A ray is eight floats (32 bytes): dir.xyz, origin.xyz, tmax, reserved.  The first six are rt_debug_trace's
 * layout; the direction is used as given, not normalised, as rayTrace uses it (MathLib.cl:234-288); reserved is
 * never read.
 *
 * RT_QUERY_CLOSEST: the hit of the reference's rayTrace under the context's "traversal" option, exactly as a
 * render sees it -- FAST: the closest triangle with the DFS-rank tie break; REF: the reference's DFS, the drops
 * beyond "ref_stack" included -- restricted to k < lim, lim = fminf(tmax, 1000.0f): a NaN tmax means 1000, the
 * reference's own horizon, and tmax <= 0 misses.  The restriction is a filter on the unrestricted closest hit:
 * that hit when its k < lim, else a miss.
 * Result: tri = the reference triangle index (the row of faceData), -1 for a miss; k = the distance, 1000.0f on a
 * miss; u, v = Moller-Trumbore's barycentrics of that triangle, recomputed once per ray after the walk in the
 * operation order of the reference's test with the IEEE 1.0f / a, 0 on a miss.
 * RT_QUERY_ANY: tri >= 0 iff the closest-hit query would hit; tri, k, u, v then describe SOME triangle the ray
 * really hits with k < lim, not necessarily the closest, and which one may differ between engines and options
 * (the persistent tree walks end at the first accepted triangle; brute force, REF and the plain form return the
 * closest).
 *
 *   rt_trace         host arrays, blocking: the rays are split in contiguous chunks over the device slots, every
 *                    slot is enqueued before any is waited for.
 *   rt_trace_device  DEVICE arrays on slot device_index, enqueued on the HIP stream `stream` (NULL = the default
 *                    stream); never waits.  d_rays and d_out must be 16-byte aligned and must not overlap.
 * A query reads the scene only: it needs no environment, leaves an open accumulation untouched and valid, and is
 * ordered with the context's other launches and uploads as a render is.
 * RT_ERR_STATE: no scene, or "traversal" is FAST and the scene has no FAST layout.  RT_ERR_ARG: n < 0, n >= 2^31,
 * a mode that is none of the two, a device index out of range, NULL arrays with n > 0, misaligned or overlapping
 * device arrays.  n == 0 is RT_OK and launches nothing. */
typedef struct { float k; int32_t tri; float u, v; } rt_hit;   /* 16 bytes */
enum rt_query_mode { RT_QUERY_CLOSEST = 0, RT_QUERY_ANY = 1 };
int rt_trace(rt_ctx* ctx, const float* rays, int64_t n, int mode, rt_hit* out);
int rt_trace_device(rt_ctx* ctx, int device_index, const float* d_rays, int64_t n, int mode, rt_hit* d_out,
                    void* stream);

/* Radiance queries: the frame's integrator (naiveGI under the sample loop, Raytracing.cl:46-151, 184-209) on the
 * caller's own rays with the caller's own RNG seeds (no counterpart in the reference, which enters it through
 * genCameraRay only).  Other cameras, depth of field, sub-pixel jitter, irradiance probes, light maps: the samples
 * are a frame's samples.  The contract: the query of a frame's camera rays with that frame's seeds is that frame,
 * bit for bit.
 *
 * A ray is eight 32-bit words (32 bytes): dir.xyz, origin.xyz -- rt_trace's first six -- then seed0, seed1 as uint
 * bits where rt_trace has tmax and reserved.  The direction is used as given wherever the reference uses R_cam.dir
 * unnormalised (rayTrace, BRDF_GGX's -R_cam.dir, the glass continuation) and normalised only where naiveGI does
 * (R_bounce.o, Raytracing.cl:79).
 * A result is the accumulation's 32-byte state record, rt_radiance_state: the sum of the samples, the first hit as
 * rt_trace reports it under the context's "traversal" (tri = the row of faceData or -1, k = the distance or 1000.0f),
 * the RNG words after the last sample and the sample count n.  The radiance is sum / (float)n; clamped to [0, 1] per
 * channel it is rt_render's pixel at spp = n when the ray is genCameraRay(i, cam) with seeds (i % npix, i / npix).
 *
 * A fresh call traces the ray, starts from sum = 0, n = 0 and the ray's seeds, runs spp samples of naiveGI with
 * max_bounce as rt_render takes it (negative: the bounce loop is never entered) and env as rt_render's, adds them in
 * order and stores the record.  With RT_RADIANCE_RESUME the record is read instead: sum, k, tri, n and the seeds come
 * from it, the ray's seed words are ignored and no first ray is traced; a stored tri outside [0, T) is a miss (and is
 * stored back as -1).  Calls of a then b samples leave the record of one call of a + b, bit for bit.  Keeping a
 * resumed ray's total at or below RT_ACCUM_MAX_SAMPLES is the caller's job: the host cannot see device records.
 * Rays with NaN or infinite components are safe: they trace as rt_trace traces them and shade without faulting.
 *
 *   rt_radiance            host arrays, blocking: contiguous chunks over the device slots, every slot enqueued
 *                          before any is waited for.
 *   rt_radiance_device     DEVICE arrays on slot device_index, enqueued on the HIP stream `stream`; never waits.
 *                          d_rays and d_state must be 16-byte aligned and must not overlap.
 *   rt_camera_rays         the rays and seeds rt_render gives pixels first .. first + count - 1 of cam's frame of
 *                          npix pixels, in the layout above (direction: genCameraRay's; origin: cam[0..2]); host
 *                          array of 8 * count floats, blocking (device 0).  Needs no scene.
 *   rt_camera_rays_device  the same into a 16-byte aligned device array, enqueued on `stream`.
 * Ordering with the context's other work follows rt_trace; a query leaves an open accumulation untouched and valid.
 * The engine: REF's DFS, brute force, or the BVH2 walk with its whole stack in LDS (the block shrinks to fit);
 * RT_ERR_SCENE when that stack does not fit a block of 64 lanes.
 * RT_ERR_STATE: no scene, no environment, or "traversal" is FAST and the scene has no FAST layout.  RT_ERR_ARG:
 * n < 0, n >= 2^31, spp < 1, spp > RT_ACCUM_MAX_SAMPLES, max_bounce > 4096, unknown flag bits, NULL arrays with
 * n > 0, misaligned or overlapping device arrays, a device index out of range; rt_camera_rays: a width below 1,
 * npix outside 1 .. 2^31 - 1, pixels outside the frame.  n == 0 (count == 0) is RT_OK and launches nothing. */
typedef struct { float sum[3]; float k; uint32_t seed0, seed1; int32_t tri; int32_t n; } rt_radiance_state; /* 32 bytes */
enum { RT_RADIANCE_RESUME = 1 };
int rt_radiance(rt_ctx* ctx, const float* rays, int64_t n, const float env[5], int spp, int max_bounce, int flags,
                rt_radiance_state* state);
int rt_radiance_device(rt_ctx* ctx, int device_index, const float* d_rays, int64_t n, const float env[5], int spp,
                       int max_bounce, int flags, rt_radiance_state* d_state, void* stream);
int rt_camera_rays(rt_ctx* ctx, const float cam[10], int64_t npix, int64_t first, int64_t count, float* rays);
int rt_camera_rays_device(rt_ctx* ctx, int device_index, const float cam[10], int64_t npix, int64_t first,
                          int64_t count, float* d_rays, void* stream);

/* Lens frames: a frame whose every sample goes down a camera ray of its own, generated on the device -- a box-filter
 * jitter of the pixel (anti-aliased edges) and a thin lens (depth of field) -- and summed into the pixel's
 * rt_radiance_state record (no counterpart in the reference, which sends all samples of a pixel down genCameraRay(i)).
 *
 * Definition of the sample ray, lens_ray(cam, lens, i, s), for pixel i and sample index s (the number of samples the
 * pixel has had, counted from 0) -- everything is fp32, evaluated in the order written, and nothing is contracted
 * except the fmafs shown:
 *   Uniforms, counter-based, uint32 arithmetic modulo 2^32:
 *          h(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *          base = h(h(seed) ^ (uint32)i) + 4 * (uint32)s
 *          u_k  = (float)(h(base + k) >> 8) * 2^-24        k = 0..3, each in [0, 1), exact
 *      The integrator's own RNG chain is not touched: a pixel keeps the frame's seeds (i % npix, i / npix), and the
 *      chain runs on from sample to sample as Raytracing.cl:171-172, 191-209 runs it.
 *   Jitter, with pixelX, pixelY, pas, position and focal as genCameraRay has them (Raytracing.cl:18-37):
 *          jx = (u0 - 0.5f) * jitter;  jy = (u1 - 0.5f) * jitter
 *          pc = ( fmaf((float)pixelY + jx, pas, -0.5f),  0,  fmaf(-((float)pixelX + jy), pas, 0.5f) )
 *          d  = normalize((position + pc) - focal)
 *      jitter is the width of a box filter in pixels; jitter == 0 adds +-0 and gives genCameraRay's bits, no branch.
 *   Lens, in the camera's local frame, before the three rotations.  aperture == 0 (a branch): the pinhole, the ray is
 *      (position, d).  Otherwise
 *          r = sqrt(u2) * aperture;  (sn, cs) = sincos(6.2831855f * u3);  l = (r * cs, 0, r * sn)
 *          t = focus / d.y;  d = normalize(d * t - l)
 *      and the origin's offset is l.  focus is the distance along the view axis (local +y) from position to the plane
 *      in focus; aperture the lens's radius.
 *   Rotations: d, and l when there is a lens, go through genCameraRay's three rotations (about x by cam[3], y by
 *      cam[4], z by cam[5]) as it applies them; the origin is position + rotated l.
 *
 * The frame: a call processes pixels first .. first + count - 1 of cam's frame of npix pixels for spp samples and
 * leaves one record per pixel.  For each sample s in order: trace lens_ray(i, s) under the context's "traversal", run
 * one naiveGI sample from that hit with the pixel's running seeds, add it to sum (a float3 add), increment n.  The
 * record: sum; seed0, seed1 the RNG words after the last sample; n; k, tri the first hit of the LAST sample's ray, as
 * rt_trace reports it.  A fresh call starts from sum = 0, n = 0 and the seeds (i % npix, i / npix).  With
 * RT_RADIANCE_RESUME sum, n and the seeds come from the record, so s continues from the record's n; tri and k of the
 * record are never read: every sample traces its own ray, no index comes from the caller's data.  The frame is
 * fmax(fmin(sum / (float)n, 1), 0) (rt_radiance_resolve_device).
 * Contracts, bit for bit:
 *   A  the record equals a sequence of S fresh rt_radiance queries at spp = 1, one per sample s = 0 .. S - 1, of the
 *      single ray lens_ray(i, s), each with the seeds the query before left (the frame's for s = 0), the sums added
 *      in order in fp32; k, tri and the seeds are the last query's;
 *   B  with jitter = 0 and aperture = 0 the records are rt_radiance's records of rt_camera_rays at the same spp, in
 *      all 32 bytes, so the frame is rt_render's;
 *   C  calls of a then b samples with RT_RADIANCE_RESUME leave the records of one call of a + b;
 *   D  the host form equals the device form, and nothing depends on "block", "radiance_grid", the engine or how the
 *      pixels are split over the device slots.
 * A camera that makes non-finite rays is safe, as non-finite rays are for rt_radiance.
 *
 *   rt_lens_radiance            host records, blocking: contiguous chunks of the pixels over the device slots, every
 *                               slot enqueued before any is waited for.
 *   rt_lens_radiance_device     DEVICE records (16-byte aligned) on slot device_index, enqueued on `stream`; never
 *                               waits.
 *   rt_lens_rays                the rays of samples sample0 .. sample0 + nsamples - 1 of the pixels, [count][nsamples][8]
 *                               floats in rt_camera_rays' layout: dir.xyz, origin.xyz, then the pixel's frame seeds,
 *                               the same for every sample, so sample 0's ray can go to rt_radiance as it is.  Host
 *                               array, blocking (device 0).  Needs no scene.
 *   rt_lens_rays_device         the same into a 16-byte aligned device array, enqueued on `stream`.
 *   rt_radiance_resolve_device  d_rgb[3 * n] = fmax(fmin(sum / (float)n, 1), 0) of n records of rt_radiance_device or
 *                               rt_lens_radiance_device, with the IEEE division (n = 0 gives NaN, which the clamp
 *                               sends to 1); enqueued on `stream`, never waits: from records to a frame, and on to
 *                               rt_rgb8_device, without the host.
 * Ordering with the context's other work follows rt_trace; a call leaves an open accumulation untouched and valid.
 * The engines and "block" / "radiance_grid" are rt_radiance's.
 * RT_ERR_STATE: no scene, no environment, or "traversal" is FAST and the scene has no FAST layout.  RT_ERR_SCENE: the
 * BVH2 stack does not fit a block of 64 lanes.  RT_ERR_ARG: rt_radiance's and rt_camera_rays' argument checks; a NULL
 * lens; a jitter or aperture that is not finite or is negative; a focus that is not finite and > 0; sample0 < 0;
 * nsamples < 1; count * nsamples >= 2^31; pixels outside the frame; misaligned device arrays (rt_radiance_resolve_
 * device: d_rgb 4-byte aligned, no overlap).  count == 0 (n == 0) is RT_OK and launches nothing. */
typedef struct { float jitter, aperture, focus; uint32_t seed; } rt_lens;   /* 16 bytes */
int rt_lens_radiance(rt_ctx* ctx, const float cam[10], const float env[5], const rt_lens* lens, int64_t npix,
                     int64_t first, int64_t count, int spp, int max_bounce, int flags, rt_radiance_state* state);
int rt_lens_radiance_device(rt_ctx* ctx, int device_index, const float cam[10], const float env[5], const rt_lens* lens,
                            int64_t npix, int64_t first, int64_t count, int spp, int max_bounce, int flags,
                            rt_radiance_state* d_state, void* stream);
int rt_lens_rays(rt_ctx* ctx, const float cam[10], const rt_lens* lens, int64_t npix, int64_t first, int64_t count,
                 int sample0, int nsamples, float* rays);
int rt_lens_rays_device(rt_ctx* ctx, int device_index, const float cam[10], const rt_lens* lens, int64_t npix,
                        int64_t first, int64_t count, int sample0, int nsamples, float* d_rays, void* stream);
int rt_radiance_resolve_device(rt_ctx* ctx, int device_index, const rt_radiance_state* d_state, int64_t n,
                               float* d_rgb, void* stream);

/* Progressive lens frames: an accumulation whose every sample goes down lens_ray(cam, lens, i, s) as above, so the
 * frames that refine, adapt and denoise get anti-aliased edges and depth of field.
 *   rt_accum_begin_lens         opens the context's one accumulation as rt_accum_begin does (replacing an open one),
 *                               every slot holding its rows of the frame;
 *   rt_accum_begin_lens_device  opens slot device_index's, of the rows row0, row0 + row_step, ..., as
 *                               rt_accum_begin_device does.  The records are initialised on the slot's own stream;
 *                               later launches on any stream are ordered after that as after any launch.
 * Every other rt_accum_* entry point works on the open accumulation, whichever kind it is: add, add_rgb8, read,
 * samples, end; mark, select, select_mask, select_all, selection, sample_map, add_selected; guides, denoise; and all
 * _device forms.  The rules above carry over unchanged: what invalidates the accumulation; that a selected add needs
 * a full add first; RT_ACCUM_MAX_SAMPLES; the tile forms enqueue on `stream` and never wait; buffers grow on first
 * use.  Of the options, "block" and "radiance_grid" apply to a lens add (the engines are rt_lens_radiance's: REF, brute
 * force, or the BVH2 walk with the whole stack in LDS); "slices", "pilot", "spec", "team", "walk_team" and "bvh_width"
 * do not.  Padding pixels of a partial last row get no sample and no ray and are never selected.
 * Contracts, bit for bit:
 *   E1  Take any sequence of full and selected adds, on any engine, block, grid, tile or split over slots.  A pixel i
 *       that has received n samples then holds the record that rt_lens_radiance returns for (cam, env, lens, npix,
 *       first = i, count = 1, spp = n, max_bounce, flags = 0), in all 32 bytes.  The frame is
 *       fmax(fmin(sum / (float)n, 1), 0) of those records.
 *   E2  With jitter = 0 and aperture = 0 every frame, sample map, selection and guide equals the plain accumulation's
 *       for the same arguments, and so the frame equals rt_render's.
 *   E3  The guides of a lens accumulation equal, in all 12 floats, the guides of a plain accumulation of the same cam,
 *       npix, scene and traversal whose pixels hold the same counts: the first hit is that of the pixel-centre pinhole
 *       ray (genCameraRay(i): rt_camera_rays' ray, traced as rt_trace traces it), whatever the lens -- a lens record's
 *       k, tri are its LAST sample's hit, not the pixel's.  The first guides call of a lens accumulation therefore
 *       traces that one ray per tile pixel into a buffer of the slot (8 bytes per pixel; dropped by begin, end and
 *       invalidation); later calls trace nothing.  The state is untouched either way: rt_accum_read before and after
 *       gives the same bits.  With aperture > 0 the guides describe the geometry in focus at the pixel's centre, so
 *       the filter under-smooths edges that are out of focus; no quality claim is made for that case.
 * Errors: rt_accum_begin's argument and state checks, then a NULL lens, a jitter or aperture that is not finite or is
 * negative, a focus that is not finite and > 0 (RT_ERR_ARG); RT_ERR_SCENE when the BVH2 stack does not fit a block of
 * 64 lanes, as for rt_lens_radiance.  A failing begin leaves things as a failing rt_accum_begin leaves them. */
int rt_accum_begin_lens(rt_ctx* ctx, const float cam[10], const float env[5], const rt_lens* lens, int64_t npix,
                        int max_bounce);
int rt_accum_begin_lens_device(rt_ctx* ctx, int device_index, const float cam[10], const float env[5],
                               const rt_lens* lens, int64_t npix, int max_bounce, int row0, int row_step);

/* Same traversal as the render, instrumented: accumulates
 * counts[0] = BVH node fetches, [1] = triangle tests, [2] = rays traced,
 * [3] = environment lookups, [4] = stack overflows (REF traversal drops),
 * for the given tile (device 0, blocking).  Feeds the algorithmic-byte
 * roofline of bench.py. */
int rt_count_work(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp,
                  int max_bounce, int row0, int row_step, uint64_t counts[5]);

/* Every counter of the instrumented render of the tile (device 0, blocking):
 * counts[0..4] as rt_count_work, [5] traversal-loop iterations per wave,
 * [6] render-loop iterations per wave, [7]/[8] clock cycles the resumable
 * kernel's waves spend shading / traversing, [9] ray-box slab tests (a FAST
 * node tests 2 boxes, a REF node 1, the brute-force path one per distinct
 * leaf box), [10]/[11]/[12] shading events (naiveGI bounces,
 * Raytracing.cl:58-78) on materials of type 1 (diffuse) / 2 (glossy) /
 * 3 (glass), [13] sun terms evaluated (Raytracing.cl:115-137), [14] samples,
 * [15] render-loop iterations per wave that handed out jobs (the brute-force
 * loops; with [6], the refill events per iteration).  Feeds the VALU roofline of bench.py. */
int rt_count_work_detail(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp,
                         int max_bounce, int row0, int row_step, uint64_t counts[16]);

/* Algorithmic bytes per unit of the counters above:
 * out[0] = 32 B per ray-box slab test (counts[9] of rt_count_work_detail:
 * a BVH2 node tests 2 child boxes, a 4-wide node up to 4, a wide leaf its
 * exact box, a REF node 1), out[1] = 36 per triangle test, out[2] = 40 per
 * ray hit record, out[3] = 16 per environment lookup. */
int rt_work_bytes(rt_ctx* ctx, double out[4]);

/* Gamma kernel of ImgProcessing.cl:1-10: out[k] = powr(min(in[k],1), 2.2)
 * for k < n, blocking, host memory. */
int rt_gamma(rt_ctx* ctx, const float* in, float* out, int64_t n);

/* Output stage (8-bit frame), replacing FileManager.saveImg's quantization
 * (FileManager.py:334-336: (data*255).astype('uint8')) and, with gamma = 1,
 * the ImgProcessing.cl gamma applied first (KernelLauncher.launch_ImgProcessing,
 * KernelLauncher.py:90-103): out[k] = (uint8)(v * 255) with v = in[k] or
 * powr(min(in[k],1), 2.2).  Exact truncation for v*255 in [0, 256) -- every
 * rendered value, the frame being clamped to [0,1]; saturating outside it
 * (NaN -> 0).
 *   rt_render_rgb8: rt_render, then quantize on the device(s); 3*npix bytes
 *                   (row-major RGB) into caller-owned host memory, blocking.
 *   rt_rgb8_device: quantize device memory d_in[n] -> d_out[n] on device
 *                   device_index, enqueued on `stream` (the gather of the
 *                   multi-process path moves these bytes); d_in 16-byte and
 *                   d_out 4-byte aligned.
 *   rt_rgb8:        host memory in -> out, blocking (device 0). */
int rt_render_rgb8(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp,
                   int max_bounce, int gamma, uint8_t* out_rgb8);
int rt_rgb8_device(rt_ctx* ctx, int device_index, const float* d_in, uint8_t* d_out, int64_t n,
                   int gamma, void* stream);
int rt_rgb8(rt_ctx* ctx, const float* in, uint8_t* out, int64_t n, int gamma);

/* BVH.py export built natively (bit-identical, see bvh_build.cpp):
 * out must hold 9*(2T-1) floats, T = nface/10; *out_nodes = nodes written. */
int rt_bvh_build(const int32_t* face, int64_t nface, const float* vp, int64_t nvp,
                 float* out, int64_t* out_nodes);

/* Device count visible to HIP (0 when no GPU). */
int rt_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_API_H */
