// C-ABI of the MI355X path tracer (include/rt_api.h, include/rt_debug.h).
//
// Replaces the pyopencl side of the reference's KernelLauncher
// (KernelLauncher.py:8-103): device selection, buffer/image uploads, the
// kernel enqueue and the blocking read-back.  Scene arrays arrive in the
// reference's flat AoS layouts (FileManager.Scene / BVH.exportArray) and are
// repacked here into the device layout of rt_internal.h:
//   * triangles pre-gathered (a.p, e1, e2) + hit record (a.n, material),
//   * BVH2 nodes holding both child boxes in BFS order (FAST traversal),
//   * the untouched 9-float export (REF traversal).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt_api.h"
#include "../../include/rt_debug.h"
#include "rt_internal.h"
#include "scene_pack.h"

// FAST tree walk: resumable traversal threshold (rt_set_option "resume_min"; -1 = auto), out of 64
// lanes still rendering: 36 on the BVH2 walk (C3 / C4 ms at 32 / 36 / 40: 138.8 / 136.8 / 136.5,
// 446.8 / 452.6 / 455.0), 48 on the 4-wide walk (C5 at 40 / 48 / 52: 5,805 / 5,705 / 5,772)
constexpr int kResumeMinBvh2 = 36, kResumeMinWide = 48;
// Denoise filter: the pass at step 1 stages its tile in LDS (rt_set_option "denoise_lds"; -1 = auto); every
// other pass reads its taps from global memory.  5 passes, ms: C2's frame 0.394 -> 0.371, C4's 0.298 -> 0.293;
// the pass at step 2 tiled the same way is slower than its taps from global memory
constexpr int kDenoiseLds = 1;

using rt::HostScene;

namespace {

thread_local std::string g_thread_error;

// A device allocation that frees itself: whoever lets one go (grow, release, ~Device) has the device selected
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct Device {
    int id = 0;
    hipStream_t stream = nullptr;
    int cus = 0;                  // compute units (sizes the FAST stack overflow buffer)
    DevBuf stack_ovf;             // FAST traversal stack entries beyond the LDS part
    DevBuf nodes, wnodes, wleaves, tri_fast, brute, brute_box, brute_cbox, brute_crow, bvh9, tri_geo, tri_shade, tri_frame, mat, ibl, ibl_sum, out, out8, counts, work, scratch_a, scratch_b;
    DevBuf pilot;                 // two-pass launches: per-pixel state, cost and order (FrameParams::pilot_*)
    rt::PilotNote pilot_note;     // ... and what the slot's last render launch did with it (rt_debug_last_pilot)
    DevBuf spec;                  // speculation: the trails' sample logs (FrameParams::spec_log)
    DevBuf slice;                 // sample slices: per-pixel state + samples done (FrameParams::slice_*)
    // Progressive accumulation of this slot's tile (rt_accum_*): the per-pixel state in a buffer of its own
    // (FrameParams::accum_state) -- no other entry point touches it -- and the frame it accumulates
    DevBuf accum;
    bool acc_open = false;
    bool acc_valid = false;       // false once the scene, the environment or the hits' definition changed
    float acc_cam[10] = {0}, acc_env[5] = {0};
    int64_t acc_npix = 0, acc_nloc = 0, acc_samples = 0;
    int acc_max_bounce = 0, acc_row0 = 0, acc_row_step = 1;
    // A lens accumulation (rt_accum_begin_lens*): every sample down lens_ray(cam, acc_lens_opt, i, s), the state
    // initialised by begin so that every add resumes.  centre: the first hit of every tile pixel's pixel-centre
    // pinhole ray, (k, tri) in 8 bytes, which the guides read (a lens record's k, tri are its last sample's);
    // traced by the first rt_accum_guides* of the accumulation, dropped by begin, end and invalidation
    bool acc_lens = false;
    rt::LensOptions acc_lens_opt{};
    DevBuf centre;
    bool acc_centre_ready = false;
    // Adaptive sampling (rt_accum_mark, rt_accum_select*, rt_accum_add_selected), each buffer allocated on first
    // use: the snapshot (acc.xyz, s: 16 bytes per pixel); the selection (SelView: list, length, compaction
    // scratch, 0/1 flags); and the list of every pixel, for a full add once the counts differ.  acc_samples is
    // then the largest count a pixel can hold (full adds + every selected add), acc_full the full adds' samples.
    DevBuf mark, sel, all;
    bool acc_marked = false, acc_selected = false, acc_all_ready = false;
    bool acc_uniform = true;      // every pixel holds acc_samples samples
    bool sel_all = false;         // the selection is rt_accum_select_all's
    int64_t sel_known = -1;       // the selection's length where the host knows it (the host forms), else -1
    int64_t acc_full = 0;
    // Denoised previews (rt_accum_guides*, rt_denoise_device, rt_accum_denoise), each allocated on first use: the
    // filter's scratch (X twice, N, P: 64 bytes per frame pixel) and the launch constants of the guide kernel;
    // the host forms' guides of this slot's tile; and, on the slot that filters, the frame-shaped input and output
    DevBuf dn, dn_const, guides, dn_rgb, dn_guides, dn_out;
    // Temporal reprojection's host form (rt_accum_reproject) and rt_denoise, on the slot that runs them, each
    // allocated on first use: the caller's previous frame and guides, and the reprojected guides (the frame goes
    // through dn_out)
    DevBuf rp_rgb, rp_guides, rp_out_guides;
    // Ray queries (rt_trace*): the hand-out counter of the persistent kernels and, for the host form, this slot's
    // rays and results -- buffers of their own, allocated on first use
    DevBuf q_counter, q_rays, q_out;
    // Radiance queries (rt_radiance*, rt_camera_rays*): the launch's work block (hand-out counter + launch constants)
    // and, for the host form, this slot's records (its rays go through q_rays) -- allocated on first use
    DevBuf rad_work, rad_state;
    char* host_stage = nullptr;   // pinned staging for rt_render / rt_render_rgb8
    int* host_pick = nullptr;     // pinned: a two-pass launch's pass-2 pick, read back (rt::RenderPending)
    size_t host_stage_bytes = 0;
    // Every launch of this context on the device shares `work` (pixel counters + launch constants)
    // and reads the scene buffers, so launches are ordered across streams: `done` is recorded after
    // each launch on its stream `last`; a launch on another stream, and every scene / IBL upload,
    // first waits for it (order_after_last).
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool pending = false;

    Device() = default;
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    // rt_destroy has waited for the slot's work.  The device stays selected while the members go: every DevBuf
    // above frees itself, so a buffer added to this struct needs no line anywhere else
    ~Device() {
        (void)hipSetDevice(id);
        if (host_stage) (void)hipHostFree(host_stage);
        if (host_pick) (void)hipHostFree(host_pick);
        if (stream) (void)hipStreamDestroy(stream);
        if (done) (void)hipEventDestroy(done);
    }
};

}  // namespace

struct rt_ctx {
    std::vector<Device> devs;
    HostScene hs;
    bool have_scene = false;
    bool have_env = false;
    int ibl_w = 0, ibl_h = 0;
    int traversal = RT_TRAVERSAL_FAST;
    int bvh_layout = RT_BVH_SAH;
    int brute_max = RT_BRUTE_MAX_DEFAULT;
    int brute_cluster = -1;  // brute force: clustered leaf boxes (0 off, 1 force, -1 auto; option "brute_cluster")
    int brute_shell = -1;    // ... and the shell among their single slots (0 off, 1 force, -1 auto; option "brute_shell")
    int brute_near = -1;     // ... whose face tests take the packer's floor (0 off, -1 or 1 auto; option "brute_near")
    int brute_direct = -1;   // ... and whose one queue step tests a lane's first record in place (0 off, -1 or 1 auto; option "brute_direct")
    int brute_lean = -1;     // the lean loop for all-diffuse one-shot frames (0 off, -1 or 1 auto; option "brute_lean"; rt_internal.h brute_lean_frame)
    int brute_primary = -1;  // ... whose sliced launches trace their camera rays in a pre-pass (0 off, -1 or 1 auto; option "brute_primary"; rt_internal.h kBrutePrimary)
    int brute_quad = -1;     // ... and whose split walls queue one record (0 off, -1 or 1 auto; option "brute_quad")
    int resume_min = -1;
    int team = 0;  // brute-force lanes per pixel, 0 = auto
    int walk_team = 0;  // tree walk (BVH2 item steps): lanes per pixel walking each ray together, 0 = auto
    int max_waves = 0;  // persistent grid cap in waves per SIMD, 0 = occupancy limit
    int step = 0;       // tree-walk traversal loop: 0 auto, 1 one item per step, 2 descend-until-leaf rounds
    int sun_skip = 1;   // FAST: do not trace shadow rays of an unlit sun (FrameParams::sun_skip)
    int sun_any = 1;    // FAST tree walk: shadow rays end at their first hit when no material is glass
    int block = 128;
    int bvh_width = 0;  // FAST tree walk: 2 = BVH2 nodes, 4 = the 4-wide quantised layout, 0 = auto (option "bvh_width")
    int fixed_point = 1;  // sum the repeats of a sample that draws no random number (FrameParams::fixed_point)
    int sun_cache = 1;    // trace the first drawing bounce's shadow ray once per pixel (FrameParams::sun_cache)
    int pilot = -1;       // two-pass launches: pilot samples per pixel (0 = one pass, -1 = auto; FrameParams::pilot)
    int pilot_chunk = 0;  // pixels ordered together (0 = auto: 64 brute force, 1 tree walk)
    int pilot_levels = 0; // cost bins of the order (0 = auto: 256)
    int stack_lds = 0;    // FAST stack entries per lane kept in LDS (0 = auto: rt::kStackLds, kStackLdsWide)
    int ref_stack = 20;   // REF traversal stack capacity (20 = the reference's, stack.cl:4)
    int spec = -1;        // small tiles: speculative trails per pixel in pass 2 (0 = off, 2, 4 or 8, -1 = auto)
    int wdq = 1;          // 4-wide walk: origin-folded dequantisation where the builder's gap covers the frame (option "wdq")
    int handout = -1;     // pixel hand-out: 0 = interleaved chunks, 1 = a contiguous block per XCD group, -1 = auto
    int slices = -1;      // one-pass tree-walk launches: sample slices per pixel (FrameParams::slices; 0 off, -1 auto)
    int brute_refill = -1;   // one-lane brute-force kernels: free lanes a wave refills together (FrameParams::refill; -1 auto, 0 or 1 off, R)
    int denoise_lds = -1;    // the filter's pass at step 1 stages its tile in LDS (0 off, 1 on, -1 auto: kDenoiseLds)
    int query_engine = 0;    // ray queries: 0 auto, 1 the plain form, 2 the persistent form (option "query_engine")
    int query_grid = 0;      // ... at most this many blocks of the persistent form (0 auto; option "query_grid")
    int radiance_grid = 0;   // radiance queries: at most this many blocks (0 auto; option "radiance_grid")
    bool accum_host = false;   // the open accumulation is rt_accum_begin's: every slot holds its rows of one frame
    // host wall times of the last calls (rt_debug_timings), ms: rt_set_scene's validation + packing and its
    // uploads (+ the per-triangle frame kernel), rt_set_env (upload + texel-sum kernel), rt_render's
    // blocking render + read-back
    double t_pack_ms = 0, t_upload_ms = 0, t_env_ms = 0, t_render_ms = 0;
    std::string err;
};

namespace {

int set_err(rt_ctx* ctx, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    g_thread_error = buf;
    return code;
}

#define HIP_OR_RET(ctx, call)                                                                           \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return set_err((ctx), RT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));           \
    } while (0)

// The one way a buffer of a slot gets its size (at least 16 bytes: never a NULL pointer).  Growing frees the old
// allocation from the host, and the slot's last launch, on whatever stream, may still read or write it: a slot with
// a launch pending waits for it first.  Only a buffer that grows pays for that, next to its hipFree and hipMalloc;
// one that is large enough returns at the first line.
hipError_t grow(Device& d, DevBuf& b, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (b.p && b.bytes >= bytes) return hipSuccess;
    hipError_t e = d.pending ? hipEventSynchronize(d.done) : hipSuccess;
    if (e != hipSuccess) return e;
    if (b.p && (e = hipFree(b.p)) != hipSuccess) return e;
    b.p = nullptr;
    b.bytes = 0;
    if ((e = hipMalloc(&b.p, bytes)) == hipSuccess) b.bytes = bytes;
    return e;
}

// ... and the pinned stage of the host forms' read-back (no copy into it is in flight between two calls)
hipError_t grow_stage(Device& d, size_t bytes) {
    if (d.host_stage_bytes >= bytes) return hipSuccess;
    hipError_t e = d.host_stage ? hipHostFree(d.host_stage) : hipSuccess;
    if (e != hipSuccess) return e;
    d.host_stage = nullptr;
    d.host_stage_bytes = 0;
    if ((e = hipHostMalloc((void**)&d.host_stage, bytes, hipHostMallocDefault)) == hipSuccess) d.host_stage_bytes = bytes;
    return e;
}

}  // namespace

namespace {

// HBM part of the FAST traversal stack: (depth - kStackLdsMin) entries for every lane a
// persistent render grid can hold (option "stack_lds" may keep as few as kStackLdsMin in LDS).
constexpr int kStackLdsMin = 8;
hipError_t ensure_stack_ovf(Device& d, const HostScene& hs) {
    const int64_t extra = (int64_t)std::max(hs.depth, hs.wdepth) - kStackLdsMin;
    if (extra <= 0) return hipSuccess;
    return grow(d, d.stack_ovf, (size_t)std::max(d.cus, 1) * rt::kMaxLanesPerCu * (size_t)extra * sizeof(int2));
}

hipError_t order_after_last(Device& d, hipStream_t s) {
    if (d.pending && d.last != s) return hipStreamWaitEvent(s, d.done, 0);
    return hipSuccess;
}

hipError_t mark_launch(Device& d, hipStream_t s) {
    d.last = s;
    d.pending = true;
    return hipEventRecord(d.done, s);
}

template <typename T>
hipError_t upload(Device& d, DevBuf& b, const std::vector<T>& v) {
    const size_t bytes = v.size() * sizeof(T);
    hipError_t e = grow(d, b, bytes);
    if (e != hipSuccess || bytes == 0) return e;
    return hipMemcpyAsync(b.p, v.data(), bytes, hipMemcpyHostToDevice, d.stream);
}

// DevScene::brute_cbox: the clustered slots, then the shell's record and slots (DevScene::shell)
hipError_t upload_cbox(Device& d, const HostScene& hs) {
    if (hs.brute_shell.empty()) return upload(d, d.brute_cbox, hs.brute_cbox);
    std::vector<float> v(hs.brute_cbox);
    v.insert(v.end(), hs.brute_shell.begin(), hs.brute_shell.end());
    const hipError_t e = upload(d, d.brute_cbox, v);
    return e != hipSuccess ? e : hipStreamSynchronize(d.stream);   // v leaves scope: the copy is done first
}

// The FAST layout of a packed scene on one slot, on its stream (rt_set_scene, and the options that pack the scene
// again): uploads are ordered after the slot's last launch, and a buffer that has to grow waits for it (grow)
int upload_fast(rt_ctx* ctx, Device& d, const HostScene& hs) {
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, order_after_last(d, d.stream));
    HIP_OR_RET(ctx, upload(d, d.nodes, hs.nodes));
    HIP_OR_RET(ctx, upload(d, d.wnodes, hs.wnodes));
    HIP_OR_RET(ctx, upload(d, d.wleaves, hs.wleaves));
    HIP_OR_RET(ctx, upload(d, d.brute, hs.brute));
    HIP_OR_RET(ctx, upload(d, d.brute_box, hs.brute_box));
    HIP_OR_RET(ctx, upload_cbox(d, hs));
    HIP_OR_RET(ctx, upload(d, d.brute_crow, hs.brute_crow));
    HIP_OR_RET(ctx, upload(d, d.tri_geo, hs.tri_geo));
    HIP_OR_RET(ctx, upload(d, d.tri_fast, hs.tri_fast));
    HIP_OR_RET(ctx, ensure_stack_ovf(d, hs));
    return RT_OK;
}

int effective_traversal(const rt_ctx* ctx) {
    return (ctx->traversal == RT_TRAVERSAL_FAST && ctx->hs.fast_ok) ? RT_TRAVERSAL_FAST : RT_TRAVERSAL_REF;
}

// The 4-wide layout serves the walk when chosen, or (auto) when the BVH2 node array exceeds
// rt::kWideMinBytes.
bool use_wide(const rt_ctx* ctx) {
    if (ctx->hs.wnodes.empty() || ctx->bvh_width == 2) return false;
    return ctx->bvh_width == 4 || (size_t)ctx->hs.nnodes * 16 * rt::kNodeF4 > rt::kWideMinBytes;
}

// the resumable walk's threshold where "resume_min" leaves it to the layout
int resume_min_of(const rt_ctx* ctx) {
    return ctx->resume_min >= 0 ? ctx->resume_min : use_wide(ctx) ? kResumeMinWide : kResumeMinBvh2;
}

rt::DevScene dev_scene(const rt_ctx* ctx, const Device& d) {
    rt::DevScene s{};
    s.nodes = (const float4*)d.nodes.p;
    s.nnodes = ctx->hs.nnodes;
    s.root_ref = ctx->hs.root_ref;
    const bool wide = use_wide(ctx);
    s.wnodes = wide ? (const float4*)d.wnodes.p : nullptr;
    s.wleaves = wide ? (const float4*)d.wleaves.p : nullptr;
    s.wroot_ref = ctx->hs.wroot_ref;
    s.wdq_omax = wide ? ctx->hs.wdq_omax : 0.0f;
    for (int k = 0; k < 6; ++k) s.root_box[k] = ctx->hs.root_box[k];
    s.bvh9 = (const float*)d.bvh9.p;
    s.nbvh9 = ctx->hs.nbvh9;
    s.ref_stack = ctx->ref_stack;
    s.tri_geo = (const float4*)d.tri_geo.p;
    s.tri_fast = (const float4*)d.tri_fast.p;
    s.tri_shade = (const float4*)d.tri_shade.p;
    s.tri_frame = (const float4*)d.tri_frame.p;
    s.ntri = ctx->hs.ntri;
    s.mat = (const float*)d.mat.p;
    s.nmat = ctx->hs.nmat;
    s.ibl_sum = (const uint32_t*)d.ibl_sum.p;
    s.ibl_w = ctx->ibl_w;
    s.ibl_h = ctx->ibl_h;
    // stack sized for whichever layout the launch picks (choose_kernel takes the wide one only for the
    // resumable walk of scenes not staged in LDS)
    s.depth = wide ? std::max(ctx->hs.depth, ctx->hs.wdepth) : ctx->hs.depth;
    s.brute = (const float4*)d.brute.p;
    s.brute_box = (const float4*)d.brute_box.p;
    s.nbrute = ctx->hs.nbrute;
    s.nbox = ctx->hs.nbox;
    s.brute_cbox = (const float4*)d.brute_cbox.p;
    s.brute_crow = (const float4*)d.brute_crow.p;
    s.ncluster = ctx->hs.ncluster;
    s.ncslot = (int32_t)(ctx->hs.brute_cbox.size() / 8);
    s.nsingle4 = s.ncslot - rt::kClusterSlots * s.ncluster;
    s.host_flags = (ctx->brute_cluster < 0 ? rt::kHostClusterAuto : 0) | (ctx->hs.nquad > 0 ? rt::kHostQuad : 0) |
                   (ctx->hs.nshell > 0 && ctx->brute_direct != 0 ? rt::kHostDirect : 0) |
                   (ctx->hs.diffuse_only && ctx->brute_lean != 0 ? rt::kHostLean : 0) |
                   (ctx->brute_primary != 0 ? rt::kHostPrimary : 0);
    s.nsingle = ctx->hs.nsingle;
    s.shell = ctx->hs.nshell > 0 ? 2 * s.ncslot : 0;
    s.near_floor = s.shell && ctx->brute_near != 0 ? ctx->hs.shell_floor : 0.0f;
    s.near_mask_lo = s.near_floor != 0.0f ? (uint32_t)ctx->hs.shell_mask : 0u;
    s.near_mask_hi = s.near_floor != 0.0f ? (uint32_t)(ctx->hs.shell_mask >> 32) : 0u;
    s.stack_lds = std::min<int32_t>(s.depth > 0 ? s.depth : 1,
                                    ctx->stack_lds > 0 ? ctx->stack_lds : wide ? rt::kStackLdsWide : rt::kStackLds);
    s.stack_ovf = (int2*)d.stack_ovf.p;
    return s;
}

int check_frame(rt_ctx* ctx, const float* cam, const float* env, int64_t npix, int spp, int max_bounce, int row0,
                int row_step, rt::FrameParams* fp) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (!ctx->have_scene) return set_err(ctx, RT_ERR_STATE, "rt_set_scene has not been called");
    if (!ctx->have_env) return set_err(ctx, RT_ERR_STATE, "rt_set_env has not been called");
    if (!cam || !env) return set_err(ctx, RT_ERR_ARG, "cam/env must not be NULL");
    if (!(cam[6] >= 1.0f) || !(cam[6] < 2147483648.0f))
        return set_err(ctx, RT_ERR_ARG, "cam[6] (row width) must be >= 1, got %g", (double)cam[6]);
    if (npix <= 0 || npix > 0x7fffffff) return set_err(ctx, RT_ERR_ARG, "pixel count %lld out of range", (long long)npix);
    if (spp < 0) return set_err(ctx, RT_ERR_ARG, "spp must be >= 0");
    if (row0 < 0 || row_step <= 0) return set_err(ctx, RT_ERR_ARG, "bad row tiling (%d, %d)", row0, row_step);
    if (max_bounce > 4096) return set_err(ctx, RT_ERR_ARG, "maxBounce %d > 4096", max_bounce);
    std::memcpy(fp->cam, cam, sizeof fp->cam);
    std::memcpy(fp->env, env, sizeof fp->env);
    fp->width = (int32_t)cam[6];
    fp->npix = npix;
    fp->spp = spp;
    fp->max_bounce = max_bounce;
    fp->row0 = row0;
    fp->row_step = row_step;
    fp->nloc = rt_tile_rows(npix, fp->width, row0, row_step) * fp->width;
    fp->log_pixel = -1;
    fp->resume_min = resume_min_of(ctx);
    fp->step = ctx->step;
    fp->sun_skip = (ctx->sun_skip && env[3] == 0.0f && env[4] >= 0.0f && ctx->hs.colors_finite) ? 1 : 0;
    fp->sun_any = (ctx->sun_any && !ctx->hs.has_glass) ? 1 : 0;
    fp->wide = use_wide(ctx) ? 1 : 0;
    fp->wdq = ctx->wdq;
    fp->fixed_point = ctx->fixed_point;
    fp->sun_cache = ctx->fixed_point && ctx->sun_cache ? 1 : 0;
    fp->pass = 0;
    fp->pilot = 0;
    fp->pilot_chunk = 1;
    fp->pilot_levels = 256;
    fp->pilot_state = nullptr;
    fp->pilot_draws = nullptr;
    fp->spec = 0;
    fp->spec_log = nullptr;
    fp->spec_cap = 0;
    fp->slices = 0;
    fp->refill = ctx->brute_refill;   // the option: launch_pick makes R of it (rt_internal.h brute_refill_launch)
    fp->slice_state = nullptr;
    fp->slice_ready = nullptr;
    fp->pilot_cost = nullptr;
    fp->pilot_order = nullptr;
    fp->team = ctx->team;
    fp->walk_team = ctx->walk_team;
    fp->max_waves = ctx->max_waves;
    // auto: contiguous per-XCD blocks on the 4-wide walk (C5, same-box A/B twice: 4,998 / 4,984 -> 4,952 /
    // 4,958 ms per frame; its L2-missing walk keeps neighbouring pixels on one XCD's L2), interleaved chunks
    // elsewhere (C3 / C4 -0.5 / +1 %, brute force untested)
    fp->handout = ctx->handout >= 0 ? ctx->handout : (use_wide(ctx) && effective_traversal(ctx) == RT_TRAVERSAL_FAST);
    fp->log_buf = nullptr;
    fp->log_cap = 0;
    fp->log_count = nullptr;
    return RT_OK;
}

// rt_set_scene, rt_set_env and the options that redefine a hit: an open accumulation cannot be continued
void invalidate_accum(rt_ctx* ctx) {
    for (auto& d : ctx->devs) {
        d.acc_valid = false;
        d.acc_marked = false;   // (mark and selection go with it)
        d.acc_selected = false;
        d.acc_centre_ready = false;   // (and a lens accumulation's centre hits: the scene they were traced in is gone)
    }
}

// the slot an entry point names (`what`: how that entry point spells the argument in its message)
int slot_of(rt_ctx* ctx, int device_index, Device** d, const char* what = "device index") {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (device_index < 0 || device_index >= (int)ctx->devs.size())
        return set_err(ctx, RT_ERR_ARG, "%s %d out of range", what, device_index);
    *d = &ctx->devs[device_index];
    return RT_OK;
}

// The options that pack the scene again ("bvh", "brute_max", "brute_cluster", "brute_shell", "brute_quad", "brute_direct"): the FAST layout of
// the current scene from the values as they are now, on every slot.  Without a scene there is nothing to do.
int repack_scene(rt_ctx* ctx) {
    if (!ctx->have_scene) return RT_OK;
    HostScene& hs = ctx->hs;
    std::string why;
    rt::pack_checked(hs, hs.bvh9.data(), hs.nbvh9, hs.ntri, ctx->bvh_layout, ctx->brute_max, ctx->brute_cluster,
                     ctx->brute_shell, ctx->brute_quad, why);
    rt::shell_direct(hs, ctx->brute_direct);
    for (auto& d : ctx->devs) {
        const int st = upload_fast(ctx, d, hs);
        if (st) return st;
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    }
    if (!hs.fast_ok) ctx->err = "FAST traversal unavailable (" + why + "); REF traversal will be used";
    return RT_OK;
}

// ---- rt_set_option: one row per key ----
// What a key accepts: a closed range, 0 or a closed range, or a short set
struct Accepts {
    enum Kind { kRange, kZeroOrRange, kSet } kind;
    int n;
    int64_t v[5];   // kRange, kZeroOrRange: v[0]..v[1]; kSet: the n members
    bool operator()(int64_t x) const {
        if (kind == kSet) return std::find(v, v + n, x) != v + n;
        return (kind == kZeroOrRange && x == 0) || (x >= v[0] && x <= v[1]);
    }
};
Accepts range(int64_t lo, int64_t hi) { return {Accepts::kRange, 2, {lo, hi}}; }
Accepts zero_or(int64_t lo, int64_t hi) { return {Accepts::kZeroOrRange, 2, {lo, hi}}; }
Accepts one_of(std::initializer_list<int64_t> members) {
    Accepts a{Accepts::kSet, (int)members.size(), {}};
    std::copy(members.begin(), members.end(), a.v);
    return a;
}

enum class Effect { kNone, kInvalidate, kRepack };   // after the store: nothing, invalidate_accum, repack_scene

struct Option {
    const char* key;
    int rt_ctx::*field;   // (the defaults are rt_ctx's member initialisers)
    Accepts accepts;
    std::string message;  // of a refused value
    Effect effect;
};

std::string bounds_message(const char* fmt, int a, int b = 0) {
    char buf[128];
    snprintf(buf, sizeof buf, fmt, a, b);
    return buf;
}

const std::vector<Option>& options() {
    constexpr Effect none = Effect::kNone, invalidate = Effect::kInvalidate, repack = Effect::kRepack;
    static const std::vector<Option> table = {
        {"traversal", &rt_ctx::traversal, range(RT_TRAVERSAL_FAST, RT_TRAVERSAL_REF), "traversal must be 0 (fast) or 1 (ref)", invalidate},
        // no repack and no upload: the packer decides where the floor is safe whatever the option, and the floor
        // reaches the kernels in DevScene, made for every launch (dev_scene); the frame is the same either way
        {"brute_near", &rt_ctx::brute_near, range(-1, 1), "brute_near must be -1 (auto), 0 (off) or 1 (auto)", none},
        // the lines and the enable ride in the shell's record (no DevScene field): packed and uploaded again
        {"brute_quad", &rt_ctx::brute_quad, range(-1, 1), "brute_quad must be -1 (auto), 0 (off) or 1 (auto)", repack},
        // the enable rides in the shell's record too (rt_layout.h kShellDirect)
        {"brute_direct", &rt_ctx::brute_direct, range(-1, 1), "brute_direct must be -1 (auto), 0 (off) or 1 (auto)", repack},
        // the flag reaches launch_pick in DevScene::host_flags, made for every launch: nothing is packed or uploaded
        {"brute_lean", &rt_ctx::brute_lean, range(-1, 1), "brute_lean must be -1 (auto), 0 (off) or 1 (auto)", none},
        {"brute_primary", &rt_ctx::brute_primary, range(-1, 1), "brute_primary must be -1 (auto), 0 (off) or 1 (auto)", none},
        {"bvh", &rt_ctx::bvh_layout, range(RT_BVH_REFERENCE, RT_BVH_SAH), "bvh must be 0 (reference tree) or 1 (sah)", repack},
        {"brute_cluster", &rt_ctx::brute_cluster, range(-1, 1), "brute_cluster must be -1 (auto), 0 (off) or 1 (force)", repack},
        {"brute_shell", &rt_ctx::brute_shell, range(-1, 1), "brute_shell must be -1 (auto), 0 (off) or 1 (force)", repack},
        {"brute_max", &rt_ctx::brute_max, range(0, 4096), "brute_max must be in 0..4096", repack},
        {"resume_min", &rt_ctx::resume_min, range(-1, 64), "resume_min must be -1 (auto) or 0..64", none},
        {"team", &rt_ctx::team, one_of({0, 1, 2, 4, 8}), "team must be 0 (auto), 1, 2, 4 or 8", none},
        {"walk_team", &rt_ctx::walk_team, one_of({0, 1, 2, 4, 8}), "walk_team must be 0 (auto), 1, 2, 4 or 8", none},
        {"sun_any", &rt_ctx::sun_any, range(0, 1), "sun_any must be 0 or 1", none},
        {"sun_skip", &rt_ctx::sun_skip, range(0, 1), "sun_skip must be 0 or 1", none},
        {"step", &rt_ctx::step, range(0, 2), "step must be 0 (auto), 1 (item) or 2 (round)", none},
        {"waves", &rt_ctx::max_waves, range(0, 8), "waves must be in 0..8", none},
        {"pilot", &rt_ctx::pilot, range(-1, 1 << 20), "pilot must be -1 (auto), 0 (off) or a sample count", none},
        {"pilot_chunk", &rt_ctx::pilot_chunk, range(0, 4096), "pilot_chunk must be in 0..4096 (0 = auto)", none},
        {"pilot_levels", &rt_ctx::pilot_levels, zero_or(2, 256), "pilot_levels must be 0 (auto) or 2..256", none},
        {"stack_lds", &rt_ctx::stack_lds, zero_or(kStackLdsMin, rt::kStackLds),
         bounds_message("stack_lds must be 0 (auto) or %d..%d", kStackLdsMin, rt::kStackLds), none},
        {"sun_cache", &rt_ctx::sun_cache, range(0, 1), "sun_cache must be 0 or 1", none},
        {"fixed_point", &rt_ctx::fixed_point, range(0, 1), "fixed_point must be 0 or 1", none},
        {"bvh_width", &rt_ctx::bvh_width, one_of({0, 2, 4}), "bvh_width must be 0 (auto), 2 or 4", none},
        {"ref_stack", &rt_ctx::ref_stack, range(20, 64), "ref_stack must be in 20..64 (20 = the reference's)", invalidate},
        {"slices", &rt_ctx::slices, range(-1, 16), "slices must be -1 (auto), 0 (off) or 1..16", none},
        {"brute_refill", &rt_ctx::brute_refill, range(-1, rt::kRefillMax),
         bounds_message("brute_refill must be -1 (auto), 0 or 1 (off) or 2..%d", rt::kRefillMax), none},
        {"denoise_lds", &rt_ctx::denoise_lds, range(-1, 1), "denoise_lds must be -1 (auto), 0 or 1", none},
        {"query_engine", &rt_ctx::query_engine, range(0, 2), "query_engine must be 0 (auto), 1 (plain) or 2 (persistent)", none},
        {"query_grid", &rt_ctx::query_grid, range(0, 1 << 20), "query_grid must be 0 (auto) or a block count", none},
        {"radiance_grid", &rt_ctx::radiance_grid, range(0, 1 << 20), "radiance_grid must be 0 (auto) or a block count", none},
        {"wdq", &rt_ctx::wdq, range(0, 1), "wdq must be 0 or 1", none},
        {"handout", &rt_ctx::handout, range(-1, 1), "handout must be -1 (auto), 0 or 1", none},
        {"spec", &rt_ctx::spec, one_of({-1, 0, 2, 4, 8}), "spec must be -1 (auto), 0 (off), 2, 4 or 8", none},
        {"block", &rt_ctx::block, one_of({64, 128, 256}), "block must be 64/128/256", none},
    };
    return table;
}

}  // namespace

extern "C" {

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt_create(int n_devices, const int* device_ids, rt_ctx** out) {
    if (!out) return set_err(nullptr, RT_ERR_ARG, "out must not be NULL");
    *out = nullptr;
    int avail = 0;
    hipError_t e = hipGetDeviceCount(&avail);
    if (e != hipSuccess || avail <= 0)
        return set_err(nullptr, RT_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
    if (n_devices <= 0) n_devices = 1;
    // explicit ids may repeat one GPU (KernelLauncher(device=[0, 0]): two row-interleaved slots, each
    // with its own stream and buffers); without ids the first n_devices GPUs must exist
    if (!device_ids && n_devices > avail)
        return set_err(nullptr, RT_ERR_ARG, "requested %d devices, %d available", n_devices, avail);
    if (n_devices > 64) return set_err(nullptr, RT_ERR_ARG, "at most 64 device slots, got %d", n_devices);
    rt_ctx* ctx = new rt_ctx();
    ctx->devs = std::vector<Device>(n_devices);
    for (int i = 0; i < n_devices; ++i) {
        const int id = device_ids ? device_ids[i] : i;
        if (id < 0 || id >= avail) {
            delete ctx;
            return set_err(nullptr, RT_ERR_ARG, "device id %d out of range", id);
        }
        ctx->devs[i].id = id;
        if ((e = hipSetDevice(id)) != hipSuccess ||
            (e = hipStreamCreateWithFlags(&ctx->devs[i].stream, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&ctx->devs[i].done, hipEventDisableTiming)) != hipSuccess ||
            (e = hipDeviceGetAttribute(&ctx->devs[i].cus, hipDeviceAttributeMultiprocessorCount, id)) != hipSuccess) {
            rt_destroy(ctx);
            return set_err(nullptr, RT_ERR_HIP, "device %d init failed: %s", id, hipGetErrorString(e));
        }
    }
    *out = ctx;
    return RT_OK;
}

void rt_destroy(rt_ctx* ctx) {
    if (!ctx) return;
    for (auto& d : ctx->devs) {   // every slot's work ends before ~Device lets go of what it uses
        if (hipSetDevice(d.id) != hipSuccess) continue;
        if (d.pending) (void)hipEventSynchronize(d.done);
        if (d.stream) (void)hipStreamSynchronize(d.stream);
    }
    delete ctx;
}

const char* rt_last_error(rt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_thread_error.c_str(); }

int rt_set_option(rt_ctx* ctx, const char* key, int64_t value) {
    if (!ctx || !key) return set_err(ctx, RT_ERR_ARG, "null argument");
    for (const Option& o : options()) {
        if (std::strcmp(key, o.key)) continue;
        if (!o.accepts(value)) return set_err(ctx, RT_ERR_ARG, "%s", o.message.c_str());
        ctx->*o.field = (int)value;
        if (o.effect == Effect::kInvalidate) invalidate_accum(ctx);
        return o.effect == Effect::kRepack ? repack_scene(ctx) : RT_OK;
    }
    return set_err(ctx, RT_ERR_ARG, "unknown option '%s'", key);
}

int rt_set_scene(rt_ctx* ctx, const float* vp, int64_t nvp, const float* vn, int64_t nvn, const float* vuv,
                 int64_t nvuv, const int32_t* face, int64_t nface, const float* mat, int64_t nmat, const float* bvh9,
                 int64_t nbvh) {
    (void)vuv;
    (void)nvuv;  // uv is carried by hitInfo but never consumed by the reference kernel
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    const auto t0 = std::chrono::steady_clock::now();
    HostScene hs;
    std::string msg, why;
    const int rc = rt::scene_prepare(hs, vp, nvp, vn, nvn, face, nface, mat, nmat, bvh9, nbvh, ctx->bvh_layout,
                                     ctx->brute_max, ctx->brute_cluster, ctx->brute_shell, ctx->brute_quad, msg, why);
    if (rc != RT_OK) return set_err(ctx, rc, "%s", msg.c_str());
    rt::shell_direct(hs, ctx->brute_direct);
    invalidate_accum(ctx);
    const auto t1 = std::chrono::steady_clock::now();
    for (auto& d : ctx->devs) {
        const int st = upload_fast(ctx, d, hs);
        if (st) return st;
        HIP_OR_RET(ctx, upload(d, d.bvh9, hs.bvh9));
        HIP_OR_RET(ctx, upload(d, d.tri_shade, hs.tri_shade));
        HIP_OR_RET(ctx, upload(d, d.mat, hs.mat));
        HIP_OR_RET(ctx, grow(d, d.tri_frame, (size_t)std::max<int64_t>(hs.ntri, 1) * 3 * sizeof(float4)));
        HIP_OR_RET(ctx, grow(d, d.work, rt::kWorkBytes));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    }
    ctx->hs = std::move(hs);
    for (auto& d : ctx->devs) {
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, rt::launch_prep_frames(dev_scene(ctx, d), (float4*)d.tri_frame.p, d.stream));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    }
    ctx->have_scene = true;
    ctx->t_pack_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    ctx->t_upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (!ctx->hs.fast_ok) ctx->err = "FAST traversal unavailable (" + why + "); REF traversal will be used";
    return RT_OK;
}

int rt_set_env(rt_ctx* ctx, const uint8_t* rgba, int w, int h) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (!rgba || w <= 0 || h <= 0) return set_err(ctx, RT_ERR_ARG, "bad IBL image (%d x %d)", w, h);
    const size_t bytes = (size_t)w * h * 4;
    invalidate_accum(ctx);
    const auto t0 = std::chrono::steady_clock::now();
    for (auto& d : ctx->devs) {
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, order_after_last(d, d.stream));
        HIP_OR_RET(ctx, grow(d, d.ibl, bytes));
        HIP_OR_RET(ctx, grow(d, d.ibl_sum, (size_t)(w + 1) * (size_t)(h + 1) * sizeof(uint32_t)));
        HIP_OR_RET(ctx, hipMemcpyAsync(d.ibl.p, rgba, bytes, hipMemcpyHostToDevice, d.stream));
        HIP_OR_RET(ctx, rt::launch_ibl_sum((const uchar4*)d.ibl.p, w, h, (uint32_t*)d.ibl_sum.p, d.stream));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    }
    ctx->ibl_w = w;
    ctx->ibl_h = h;
    ctx->have_env = true;
    ctx->t_env_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}

int64_t rt_tile_rows(int64_t npix, int width, int row0, int row_step) {
    if (npix <= 0 || width <= 0 || row0 < 0 || row_step <= 0) return 0;
    const int64_t H = (npix + width - 1) / width;
    if (row0 >= H) return 0;
    return (H - row0 + row_step - 1) / row_step;
}

namespace {
// Sample slices per pixel (setup_slices): auto on the 4-wide walk, and on BVH2 tiles of at least
// kSlicesMinPerLane pixels per resident lane, where they replace the two-pass pilot.  r05 (ms, pilot auto
// vs slices 8 with the pilot off; rows 0::N): C3 N=1 126.5 / 114.8, N=2 78.7 / 65.6, N=4 54.3 / 84.8
// (teams + trails); C4 N=1 303.6 / 284.8, N=2 181.5 / 254.9 (3/4 of C4's pixels are sky, finished by
// the pilot pass: the rest is one pixel per lane, where trails win), N=4 121.4 / 318.4
constexpr int kSlicesWide = 8;
constexpr int kSlicesWideSmall = 12;
constexpr int64_t kSlicesMinPerLane = 4;
using rt::kAccumSliceMin;   // (rt_slices.h, with the brute-force scenes' rule)

// Two-pass launches (FrameParams::pass): FAST tree-walk renders of tiles with more pixels than the
// device keeps lanes resident get a pilot pass of spp / 8 samples (option "pilot": -1 auto, 0 off,
// or K), whose per-pixel costs order the rest of the frame, most expensive first (rt_kernels.hip
// launch_render).  Sets fp's pilot fields and sizes the device's scratch for them.
hipError_t setup_pilot(rt_ctx* ctx, Device& d, rt::FrameParams& fp) {
    if (ctx->pilot == 0 || effective_traversal(ctx) != RT_TRAVERSAL_FAST || fp.nloc <= 0 || use_wide(ctx))
        return hipSuccess;   // (the 4-wide walk is one-pass: its pilot measured slower, r02-r03)
    int k = ctx->pilot;
    if (k < 0) {   // auto: the tree walk on tiles of 1-16 pixels per resident lane (where the tail is long)
        const int64_t lanes = (int64_t)std::max(d.cus, 1) * rt::kWalkLanesPerCu;
        // not on the 4-wide walk (C5), whose L2-missing walk loses the coherence of neighbouring pixels
        // when they are reordered: r03 row tiles 1/2, 1/4, 1/8: 3,005 / 1,626 / 937 ms without the pilot,
        // 3,185 / 1,694 / 938 with it
        if (ctx->hs.nbrute > 0 || use_wide(ctx) || fp.spp < 16 || fp.nloc > 16 * lanes) return hipSuccess;
        // tiles of kSlicesMinPerLane or more pixels per resident lane take sample slices instead (setup_slices)
        if (ctx->slices != 0 && fp.nloc >= kSlicesMinPerLane * lanes) return hipSuccess;
        // spp/8 samples, small tiles (multi-GPU row tiles, whose pass 2 takes teams or speculative trails)
        // included: r04 1/8 tiles with trails, pilot spp/16 / spp/8 / 3spp/16: C4 80.8 / 78.3 / 77.0 ms,
        // C3 35.3 / 33.9 / 35.1 ms; 1/4 tiles C4 120.7 / 119.9 / 129.1, C3 54.8 / 54.8 / 56.1 (r03, teams
        // without trails, had preferred spp/16: C3 49.3 vs 49.9, C4 142 vs 146)
        k = fp.spp / 8;
    }
    if (k >= fp.spp) return hipSuccess;
    // the state, cost and order of every pixel, the sort's scratch and the RNG offsets (rt_internal.h pilot_layout)
    const rt::PilotLayout L = rt::pilot_layout((size_t)fp.nloc);
    hipError_t e = grow(d, d.pilot, L.need);
    if (e != hipSuccess) return e;
    char* base = (char*)d.pilot.p;
    fp.pilot = k;
    fp.pilot_chunk = ctx->pilot_chunk > 0 ? ctx->pilot_chunk : (ctx->hs.nbrute > 0 ? 64 : 1);
    fp.pilot_levels = ctx->pilot_levels > 0 ? ctx->pilot_levels : 256;
    fp.pilot_state = (float4*)base;
    fp.pilot_cost = (uint32_t*)(base + L.cost);
    fp.pilot_order = (const uint32_t*)(base + L.order);
    fp.pilot_draws = (uint32_t*)(base + L.draws);
    // speculation (option "spec"): small tiles of the BVH2 walk continue as trails in pass 2
    const int64_t lanes = (int64_t)std::max(d.cus, 1) * rt::kWalkLanesPerCu;
    // up to 4 pixels per resident lane: pass 1 finishes the pixels that draw nothing (sky), and the device
    // picks trails only when the rest is at most one pixel per lane (pilot_team_pick_kernel)
    // (auto); a set trail count applies to any tile.  A trail's record count shares a word with its mode
    // (rt_spec.hip): spp < 2^16
    if (ctx->spec != 0 && (ctx->spec > 0 || fp.nloc <= 4 * lanes) && fp.spp < 65536 && !use_wide(ctx) &&
        ctx->hs.nbrute == 0) {
        fp.spec = ctx->spec;   // 2, 4 or 8 trails, or -1: chosen on the device from the pixels pass 1 left
        // records per trail: a trail t >= 1 starts t (spp - k) / T samples ahead, so it never needs more than
        // spp - k records; past kSpecCapMax it stops and the chain goes on in a trail further ahead or in
        // trail 0 (rt_spec.hip) -- the frame does not depend on the cap, the log size (CUs x lanes x cap x
        // 16 B, at most 1 GB on 256 CUs) no longer grows with spp
        fp.spec_cap = std::min(fp.spp - k, rt::kSpecCapMax);
        const size_t lbytes = rt::spec_log_bytes(fp, d.cus);
        e = grow(d, d.spec, lbytes);
        if (e != hipSuccess) {
            if (ctx->spec > 0) return e;
            // auto: a device short of memory renders pass 2 without trails (same frame) instead of failing
            (void)hipGetLastError();
            fp.spec = 0;
            fp.spec_cap = 0;
            return hipSuccess;
        }
        fp.spec_log = (float4*)d.spec.p;
    }
    return hipSuccess;
}
}  // namespace

namespace {
// Sample slices (FrameParams::slices; option "slices": -1 auto, 0 or 1 off, K): one-pass launches of the
// resumable tree walk hand out each pixel's samples as K slices, slice-major, so that a tile ends on a
// slice rather than on a whole pixel.  Auto: on the 4-wide walk (C5, whose pixels are all about equally
// long: a tile of n pixels per resident lane ends after ceil(n) pixel times, 2.26 -> 3 on an eighth of
// C5), K = kSlicesWide.  r05, C5 tiles rows 0::N (ms, K = off / 2 / 4 / 8): N=8 826 / 724 / 664 / 635,
// N=4 1,395 / 1,273 / 1,221 / 1,197, N=2 2,536 / 2,409 / 2,361 / 2,343, N=1 4,796 / 4,692 / 4,642 / 4,648
// (the wave cap of 6 instead: 838 / 1,444 / 2,651 / 5,066).  Sets fp's slice fields, sizes the device's
// state buffer and zeroes the samples-done words on stream s (the launch's stream).
// Brute-force scenes (r09): the one-lane kernels take slices too, K = kSlicesBrute on auto, decided at the launch.
hipError_t setup_slices(rt_ctx* ctx, Device& d, rt::FrameParams& fp, hipStream_t s, int accum_base = -1) {
    fp.slices = 0;
    // brute-force scenes (the one-lane kernels, render_kernel): one-pass launches; K on auto is handed on as
    // -K, and the launch decides where it knows its kernel's resident lanes (rt_kernels.hip launch_pick), which
    // also zeroes the samples-done words when it takes slices
    const bool brute = ctx->hs.nbrute > 0;
    if (effective_traversal(ctx) != RT_TRAVERSAL_FAST || fp.nloc <= 0 || ctx->slices == 0 ||
        (brute ? fp.pilot > 0 : fp.resume_min <= 0))
        return hipSuccess;
    const int64_t lanes = (int64_t)std::max(d.cus, 1) * rt::kWalkLanesPerCu;
    // pilot launches: pass 2 slices the samples after the pilot's when the device gives it one lane per pixel
    // (pilot_team_pick_kernel: more unfinished pixels than lanes); the team and trail kernels take none
    int k = ctx->slices > 0 ? ctx->slices
            : brute        ? rt::kSlicesBrute
                           : (use_wide(ctx) || fp.pilot > 0 || fp.nloc >= kSlicesMinPerLane * lanes) ? kSlicesWide : 1;
    // the 4-wide walk's small tiles (under kSlicesMinPerLane pixels per resident lane: C5's eighth, 2.26) take
    // finer slices: 1/8 tile 629.7 / 620.8 ms at 8 / 12 (whole frame 4,594 / 4,612: 8 kept there)
    if (ctx->slices < 0 && !brute && use_wide(ctx) &&
        fp.nloc < kSlicesMinPerLane * (int64_t)std::max(d.cus, 1) * rt::kWideWaves * 4 * 64)
        k = kSlicesWideSmall;
    // every slice at least two samples; accum_base >= 0: an add of a progressive accumulation, whose slices
    // split the samples it adds -- chosen automatically, at least kAccumSliceMin each (below that the
    // hand-offs cost more than the shorter tail gives back)
    const int todo = fp.spp - std::max(fp.pilot, 0) - std::max(accum_base, 0);
    k = std::min(k, todo / 2);
    if (accum_base >= 0 && ctx->slices < 0) k = std::min(k, todo / kAccumSliceMin);
    // brute-force scenes: the same bounds, from the rule the tests evaluate (rt_slices.h); K on auto goes on as -K
    const int offer = brute ? rt::brute_slice_offer(ctx->slices, todo, accum_base >= 0) : 0;
    if (brute) k = offer < 0 ? -offer : offer;
    if (k <= 1 || (int64_t)fp.nloc * (k + (brute ? 1 : 0)) >= ((int64_t)1 << 32))
        return hipSuccess;   // (the hand-out's job counters fit a word: take_pixel, take_job)
    const size_t n = (size_t)fp.nloc;
    const size_t sbytes = brute ? 48 : 32;   // (the brute-force kernels' state carries the camera ray, slice_publish)
    const size_t need = n * sbytes + n * sizeof(uint32_t);
    hipError_t e = grow(d, d.slice, need);
    if (e == hipSuccess && !brute) e = hipMemsetAsync((char*)d.slice.p + n * sbytes, 0, n * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    fp.slices = brute ? offer : k;
    fp.slice_state = (float4*)d.slice.p;
    fp.slice_ready = (uint32_t*)((char*)d.slice.p + n * sbytes);
    return hipSuccess;
}

}  // namespace

int rt_render_device(rt_ctx* ctx, int device_index, const float cam[10], const float env[5], int64_t npix, int spp,
                     int max_bounce, int row0, int row_step, float* d_out, void* stream) {
    rt::FrameParams fp;
    Device* dp = nullptr;
    int st = check_frame(ctx, cam, env, npix, spp, max_bounce, row0, row_step, &fp);
    if (!st) st = slot_of(ctx, device_index, &dp);
    if (st) return st;
    if (!d_out && fp.nloc > 0) return set_err(ctx, RT_ERR_ARG, "d_out must not be NULL");
    Device& d = *dp;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    hipStream_t s = (hipStream_t)stream;  // NULL = the device's default (null) stream, HIP convention
    HIP_OR_RET(ctx, order_after_last(d, s));
    HIP_OR_RET(ctx, setup_pilot(ctx, d, fp));
    HIP_OR_RET(ctx, setup_slices(ctx, d, fp, s));
    HIP_OR_RET(ctx, rt::launch_render(dev_scene(ctx, d), fp, effective_traversal(ctx), ctx->block, d_out, nullptr,
                                      (unsigned int*)d.work.p, s, nullptr, &d.pilot_note));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}

namespace {
// The host half of the read-back: the pinned stage into the caller's (pageable) array, split over up
// to 8 threads for frames of several MB (C2's 12.6 MB: one thread ~0.6 ms, the memory bus takes more
// from several).
void par_copy(char* dst, const char* src, size_t n) {
    constexpr size_t kPiece = 2u << 20;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t k = std::min<size_t>(std::min(8u, hw), n / kPiece);
    if (k <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    const size_t chunk = ((n + k - 1) / k + 4095) & ~(size_t)4095;
    std::vector<std::thread> ts;
    size_t i = 1;
    // a thread that cannot be created (a thread / cgroup limit) must not throw across the C ABI: the
    // chunks no thread took are copied here
    try {
        for (; i < k && i * chunk < n; ++i)
            ts.emplace_back([=] { std::memcpy(dst + i * chunk, src + i * chunk, std::min(chunk, n - i * chunk)); });
    } catch (...) {
    }
    for (size_t r = i; r < k && r * chunk < n; ++r) std::memcpy(dst + r * chunk, src + r * chunk, std::min(chunk, n - r * chunk));
    std::memcpy(dst, src, std::min(chunk, n));
    for (auto& t : ts) t.join();
}

// Rows of a frame over the slots: frame row r is row r / nd of slot r % nd's tile, and the frame's last row may be
// partial.  gather_rows: slot k's tile-packed array (elem bytes per pixel) into the frame's order.  (static: these
// unnamed namespaces open inside extern "C", where a function's C name stays a dynamic symbol without it)
static void gather_rows(char* frame, const char* tile, size_t elem, int k, int nd, int W, int64_t npix) {
    const int64_t rows = rt_tile_rows(npix, W, k, nd);
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t first = ((int64_t)k + r * nd) * W;
        std::memcpy(frame + first * elem, tile + r * W * elem, (size_t)std::min<int64_t>(W, npix - first) * elem);
    }
}
// ... and scatter_rows, its inverse: slot k's rows out of a frame-ordered array, tile-packed
static void scatter_rows(char* tile, const char* frame, size_t elem, int k, int nd, int W, int64_t npix) {
    const int64_t rows = rt_tile_rows(npix, W, k, nd);
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t first = ((int64_t)k + r * nd) * W;
        std::memcpy(tile + r * W * elem, frame + first * elem, (size_t)std::min<int64_t>(W, npix - first) * elem);
    }
}

// The read-back of the host forms, after every slot's frame is enqueued into its d.out.  Enqueue: the slot's nloc
// pixels into its pinned stage (grow_stage came first), for rgb8 >= 0 quantised on the device (rgb8 = 1: gamma
// first), so that 1 byte per channel crosses PCIe
static int readback_enqueue(rt_ctx* ctx, Device& d, int64_t nloc, int rgb8) {
    const size_t bytes = (size_t)nloc * 3 * (rgb8 >= 0 ? 1 : sizeof(float));
    const void* src = d.out.p;
    if (rgb8 >= 0) {
        HIP_OR_RET(ctx, grow(d, d.out8, bytes));
        HIP_OR_RET(ctx, rt::launch_rgb8((const float*)d.out.p, (uint8_t*)d.out8.p, nloc * 3, rgb8 == 1, d.stream));
        src = d.out8.p;
    }
    HIP_OR_RET(ctx, hipMemcpyAsync(d.host_stage, src, bytes, hipMemcpyDeviceToHost, d.stream));
    return RT_OK;
}
// Finish: wait for every slot; then (out != NULL) the stages into out, elem bytes per channel: one slot's stage is
// the frame, several slots' are gathered row by row
static int readback_finish(rt_ctx* ctx, void* out, size_t elem, int64_t npix, int W) {
    const int nd = (int)ctx->devs.size();
    for (int k = 0; k < nd; ++k) {
        Device& d = ctx->devs[k];
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
        if (!out) continue;
        if (nd == 1) par_copy((char*)out, d.host_stage, (size_t)npix * 3 * elem);
        else gather_rows((char*)out, d.host_stage, 3 * elem, k, nd, W, npix);
    }
    return RT_OK;
}

// rt_render / rt_render_rgb8: every device renders its rows (row r on device r mod n), then the read-back above
// (rgb8 as there; < 0: the float frame)
int render_host_(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp, int max_bounce,
                 void* out, int rgb8) {
    rt::FrameParams fp0;
    int st = check_frame(ctx, cam, env, npix, spp, max_bounce, 0, 1, &fp0);
    if (st) return st;
    if (!out) return set_err(ctx, RT_ERR_ARG, "output must not be NULL");
    const int nd = (int)ctx->devs.size();
    const int W = fp0.width;
    const size_t elem = rgb8 >= 0 ? 1 : sizeof(float);
    // Launch every device, then read back: devices run concurrently.  A two-pass launch's second pass
    // waits for the device's pick after its first pass (rt::RenderPending): every device's first pass is
    // enqueued before the host waits for any.
    std::vector<rt::RenderPending> pend(nd);
    for (int k = 0; k < nd; ++k) {
        Device& d = ctx->devs[k];
        rt::FrameParams fp = fp0;
        fp.row0 = k;
        fp.row_step = nd;
        fp.nloc = rt_tile_rows(npix, W, k, nd) * W;
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        if (fp.nloc == 0) continue;
        HIP_OR_RET(ctx, grow(d, d.out, (size_t)fp.nloc * 3 * sizeof(float)));
        HIP_OR_RET(ctx, grow_stage(d, (size_t)fp.nloc * 3 * elem));
        HIP_OR_RET(ctx, order_after_last(d, d.stream));
        HIP_OR_RET(ctx, setup_pilot(ctx, d, fp));
        HIP_OR_RET(ctx, setup_slices(ctx, d, fp, d.stream));
        if (!d.host_pick) HIP_OR_RET(ctx, hipHostMalloc((void**)&d.host_pick, sizeof(int), hipHostMallocDefault));
        pend[k].host_pick = d.host_pick;
        HIP_OR_RET(ctx, rt::launch_render(dev_scene(ctx, d), fp, effective_traversal(ctx), ctx->block,
                                          (float*)d.out.p, nullptr, (unsigned int*)d.work.p, d.stream, &pend[k],
                                          &d.pilot_note));
        HIP_OR_RET(ctx, mark_launch(d, d.stream));   // (again after pass 2 below; an error in between leaves it ordered)
    }
    for (int k = 0; k < nd; ++k) {
        Device& d = ctx->devs[k];
        const int64_t nloc = rt_tile_rows(npix, W, k, nd) * W;
        if (nloc == 0) continue;
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, rt::launch_render_finish(dev_scene(ctx, d), effective_traversal(ctx), ctx->block,
                                                 (float*)d.out.p, (unsigned int*)d.work.p, d.stream, pend[k]));
        HIP_OR_RET(ctx, mark_launch(d, d.stream));
        st = readback_enqueue(ctx, d, nloc, rgb8);
        if (st) return st;
    }
    return readback_finish(ctx, out, elem, npix, W);
}

int render_host(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp, int max_bounce,
                void* out, int rgb8) {
    const auto t0 = std::chrono::steady_clock::now();
    const int st = render_host_(ctx, cam, env, npix, spp, max_bounce, out, rgb8);
    if (ctx) ctx->t_render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
}

// What a launch of the radiance and lens kernels takes from the context: the render loop's exact shortcuts under the
// conditions check_frame sets them (a lens launch drops fixed_point and sun_cache unless the lens is degenerate)
rt::RadianceOptions radiance_options(const rt_ctx* ctx, const float env[5], int spp, int max_bounce, int flags) {
    rt::RadianceOptions q{};
    std::memcpy(q.env, env, sizeof q.env);
    q.spp = spp;
    q.max_bounce = max_bounce;
    q.flags = (flags & RT_RADIANCE_RESUME ? 1 : 0) |
              (ctx->sun_skip && env[3] == 0.0f && env[4] >= 0.0f && ctx->hs.colors_finite ? 2 : 0) |
              (ctx->fixed_point ? 4 : 0) | (ctx->fixed_point && ctx->sun_cache ? 8 : 0);
    q.grid_cap = ctx->radiance_grid;
    q.max_waves = ctx->max_waves;
    q.block = ctx->block;
    return q;
}

int lens_check(rt_ctx* ctx, const rt_lens* lens);   // (with the lens frames, below)
rt::LensOptions lens_options(const rt_lens* lens);

// ---- progressive accumulation (rt_accum_*) ----
// begin and end: no mark, no selection, every pixel at the same count
void accum_reset_selection(Device& d) {
    d.acc_marked = false;
    d.acc_selected = false;
    d.acc_all_ready = false;
    d.acc_uniform = true;
    d.sel_all = false;
    d.sel_known = -1;
    d.acc_full = 0;
}

int accum_close_slot(rt_ctx* ctx, Device& d) {
    d.acc_open = false;
    d.acc_valid = false;
    d.acc_samples = 0;
    d.acc_lens = false;
    d.acc_centre_ready = false;
    accum_reset_selection(d);
    if (!d.accum.p && !d.mark.p && !d.sel.p && !d.all.p && !d.centre.p) return RT_OK;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    if (d.pending) HIP_OR_RET(ctx, hipEventSynchronize(d.done));   // an add in flight still uses the state
    for (DevBuf* b : {&d.accum, &d.mark, &d.sel, &d.all, &d.centre}) b->release();
    return RT_OK;
}

// the host forms: the open accumulation is rt_accum_begin's (every slot holds its rows of one frame)
static int accum_host_open(rt_ctx* ctx, const char* what) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (!ctx->accum_host || ctx->devs.empty() || !ctx->devs[0].acc_open)
        return set_err(ctx, RT_ERR_STATE, "%s: no accumulation is open (rt_accum_begin)", what);
    return RT_OK;
}

int accum_slot_usable(rt_ctx* ctx, const Device& d, const char* what) {
    if (!d.acc_open) return set_err(ctx, RT_ERR_STATE, "%s: no accumulation is open", what);
    if (!d.acc_valid)
        return set_err(ctx, RT_ERR_STATE, "%s: the accumulation was invalidated (scene, environment, \"traversal\" "
                       "or \"ref_stack\" changed since it began)", what);
    return RT_OK;
}

int accum_check_add(rt_ctx* ctx, const Device& d, int spp) {
    int st = accum_slot_usable(ctx, d, "rt_accum_add");
    if (st) return st;
    if (spp < 1) return set_err(ctx, RT_ERR_ARG, "rt_accum_add: spp must be >= 1, got %d", spp);
    if (d.acc_samples + (int64_t)spp > RT_ACCUM_MAX_SAMPLES)
        return set_err(ctx, RT_ERR_ARG, "rt_accum_add: %lld + %d samples exceed RT_ACCUM_MAX_SAMPLES (%d)",
                       (long long)d.acc_samples, spp, (int)RT_ACCUM_MAX_SAMPLES);
    return RT_OK;
}

// rt_accum_add_selected: the slot has a selection, every pixel at least one sample (a full add), and no
// selected pixel would pass the limit -- compared against acc_samples, the most any pixel holds
int accum_check_add_selected(rt_ctx* ctx, const Device& d, int spp) {
    const char* what = "rt_accum_add_selected";
    int st = accum_slot_usable(ctx, d, what);
    if (st) return st;
    if (!d.acc_selected) return set_err(ctx, RT_ERR_STATE, "%s: no selection (rt_accum_select*)", what);
    if (d.acc_full < 1)
        return set_err(ctx, RT_ERR_STATE, "%s: the accumulation has no full add yet (rt_accum_add)", what);
    if (spp < 1) return set_err(ctx, RT_ERR_ARG, "%s: spp must be >= 1, got %d", what, spp);
    if (d.acc_samples + (int64_t)spp > RT_ACCUM_MAX_SAMPLES)
        return set_err(ctx, RT_ERR_ARG, "%s: %lld + %d samples exceed RT_ACCUM_MAX_SAMPLES (%d)", what,
                       (long long)d.acc_samples, spp, (int)RT_ACCUM_MAX_SAMPLES);
    return RT_OK;
}

// the selection's buffer (Device::sel) of a tile of n pixels: the list, its length, the compaction's scratch
// (both device words), the 0/1 flags the list was compacted from (rt_accum_selection reads them back)
struct SelView {
    uint32_t* list;
    uint32_t* count;
    uint32_t* scratch;
    uint8_t* flag;
};
size_t sel_bytes(int64_t n) { return (size_t)n * 4 + 4 + rt::select_scratch_words(n) * 4 + (size_t)n; }
SelView sel_view(const Device& d) {
    const size_t n = (size_t)d.acc_nloc;
    char* b = (char*)d.sel.p;
    return {(uint32_t*)b, (uint32_t*)(b + n * 4), (uint32_t*)(b + n * 4 + 4),
            (uint8_t*)(b + n * 4 + 4 + rt::select_scratch_words(d.acc_nloc) * 4)};
}

// the slot's tile as check_frame describes it (row tiling, width, npix), for the select kernels
void accum_tile(const Device& d, rt::FrameParams& fp) {
    fp = rt::FrameParams{};
    fp.width = (int32_t)d.acc_cam[6];
    fp.npix = d.acc_npix;
    fp.row0 = d.acc_row0;
    fp.row_step = d.acc_row_step;
    fp.nloc = d.acc_nloc;
}

// the slot, its accumulation usable and holding samples
int accum_slot_of(rt_ctx* ctx, int device_index, const char* what, Device** out) {
    int st = slot_of(ctx, device_index, out);
    if (!st) st = accum_slot_usable(ctx, **out, what);
    if (st) return st;
    if ((*out)->acc_samples == 0) return set_err(ctx, RT_ERR_STATE, "%s: the accumulation has no samples yet", what);
    return RT_OK;
}

// flags -> the ordered list (what: 0 the error measure against the mark, 1 a tile-packed device mask, 2 all)
int accum_select_slot(rt_ctx* ctx, Device& d, int what, float threshold, const uint8_t* d_mask, hipStream_t s) {
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, grow(d, d.sel, sel_bytes(d.acc_nloc)));
    const SelView v = sel_view(d);
    rt::FrameParams fp;
    accum_tile(d, fp);
    HIP_OR_RET(ctx, order_after_last(d, s));
    d.acc_selected = false;   // (an error below leaves the list undefined)
    if (what == 0)
        HIP_OR_RET(ctx, rt::launch_select_error((const float4*)d.accum.p, (const float4*)d.mark.p, v.flag, fp, threshold, s));
    else
        HIP_OR_RET(ctx, rt::launch_select_mask(what == 1 ? d_mask : nullptr, v.flag, fp, s));
    HIP_OR_RET(ctx, rt::launch_select_compact(v.flag, d.acc_nloc, v.scratch, v.list, v.count, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    d.acc_selected = true;
    d.sel_all = what == 2;
    d.sel_known = -1;
    return RT_OK;
}

// the host forms of the selects: every slot's select on its own stream, then the lengths read back
int accum_select_host(rt_ctx* ctx, int what, float threshold, const uint8_t* mask, int64_t* n_selected,
                      const char* name) {
    const int open = accum_host_open(ctx, name);
    if (open) return open;
    if (what == 1 && !mask) return set_err(ctx, RT_ERR_ARG, "%s: mask must not be NULL", name);
    const int nd = (int)ctx->devs.size();
    for (int k = 0; k < nd; ++k) {
        Device* d = nullptr;
        const int st = accum_slot_of(ctx, k, name, &d);
        if (st) return st;
        if (what == 0 && !d->acc_marked) return set_err(ctx, RT_ERR_STATE, "%s: no mark (rt_accum_mark)", name);
    }
    const int64_t npix = ctx->devs[0].acc_npix;
    const int W = (int)ctx->devs[0].acc_cam[6];
    std::vector<std::vector<uint8_t>> tiles(nd);   // (kept until the copies are done)
    for (int k = 0; k < nd; ++k) {
        Device& d = ctx->devs[k];
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        const uint8_t* d_mask = nullptr;
        if (what == 1 && d.acc_nloc > 0) {   // the slot's rows of the mask, tile-packed, staged in d.out8
            tiles[k].assign((size_t)d.acc_nloc, 0);
            scatter_rows((char*)tiles[k].data(), (const char*)mask, 1, k, nd, W, npix);
            HIP_OR_RET(ctx, grow(d, d.out8, (size_t)d.acc_nloc));
            HIP_OR_RET(ctx, order_after_last(d, d.stream));
            HIP_OR_RET(ctx, hipMemcpyAsync(d.out8.p, tiles[k].data(), (size_t)d.acc_nloc, hipMemcpyHostToDevice, d.stream));
            d_mask = (const uint8_t*)d.out8.p;
        }
        const int st = accum_select_slot(ctx, d, what, threshold, d_mask, d.stream);
        if (st) return st;
    }
    int64_t total = 0;
    for (int k = 0; k < nd; ++k) {
        Device& d = ctx->devs[k];
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        uint32_t n = 0;
        HIP_OR_RET(ctx, hipMemcpyAsync(&n, sel_view(d).count, sizeof n, hipMemcpyDeviceToHost, d.stream));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
        d.sel_known = n;
        total += n;
    }
    if (n_selected) *n_selected = total;
    return RT_OK;
}

// a per-pixel array of every slot (elem bytes per pixel, tile-packed at src(d)) gathered into the frame's order
int accum_gather_host(rt_ctx* ctx, void* out, size_t elem, const void* (*src)(Device&)) {
    const int nd = (int)ctx->devs.size();
    const int64_t npix = ctx->devs[0].acc_npix;
    const int W = (int)ctx->devs[0].acc_cam[6];
    std::vector<char> tile;
    for (int k = 0; k < nd; ++k) {
        Device& d = ctx->devs[k];
        if (d.acc_nloc <= 0) continue;
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        tile.resize((size_t)d.acc_nloc * elem);
        HIP_OR_RET(ctx, order_after_last(d, d.stream));
        HIP_OR_RET(ctx, hipMemcpyAsync(tile.data(), src(d), tile.size(), hipMemcpyDeviceToHost, d.stream));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
        gather_rows((char*)out, tile.data(), elem, k, nd, W, npix);
    }
    return RT_OK;
}

// the lens kernels keep a lane's whole traversal stack in LDS (rt_lens_radiance's rule)
int lens_fits(rt_ctx* ctx, const rt::DevScene& sc, const char* what) {
    const int trav = effective_traversal(ctx);
    if (rt::radiance_fits(sc, trav, ctx->block)) return RT_OK;
    return set_err(ctx, RT_ERR_SCENE, "%s: a traversal stack of %d entries per lane does not fit a block of 64 lanes",
                   what, trav == RT_TRAVERSAL_REF ? (int)sc.ref_stack : (int)sc.depth);
}

// An add of a lens accumulation, on the stream the caller has ordered: spp samples of every tile pixel (list NULL)
// or of the listed ones, each from its record's own count (the caller resolves the frame from the state)
int accum_add_lens(rt_ctx* ctx, Device& d, const rt::FrameParams& fp, int spp, const uint32_t* list,
                   const uint32_t* count, hipStream_t s) {
    const rt::DevScene sc = dev_scene(ctx, d);
    const rt::RadianceOptions q = radiance_options(ctx, d.acc_env, spp, d.acc_max_bounce, RT_RADIANCE_RESUME);
    d.acc_valid = false;   // (an error below leaves the state undefined)
    HIP_OR_RET(ctx, rt::launch_lens_accum(sc, effective_traversal(ctx), fp, (float4*)d.accum.p, list, count,
                                          d.acc_lens_opt, q, d.rad_work.p, s));
    d.acc_valid = true;
    return RT_OK;
}

// the host forms: add spp samples on every slot (read: resolve the state instead, nothing rendered), then read
// the frame back as render_host_ does (rgb8 >= 0: quantised on the devices first); out may be NULL for an add
// (selected: rt_accum_add_selected -- the add runs on each slot's selection)
int accum_host(rt_ctx* ctx, int spp, bool read, void* out, int rgb8, const char* what, bool selected = false) {
    const int open = accum_host_open(ctx, what);
    if (open) return open;
    const int nd = (int)ctx->devs.size();
    for (int k = 0; k < nd; ++k) {
        const int st = read       ? accum_slot_usable(ctx, ctx->devs[k], what)
                       : selected ? accum_check_add_selected(ctx, ctx->devs[k], spp)
                                  : accum_check_add(ctx, ctx->devs[k], spp);
        if (st) return st;
    }
    if (read && ctx->devs[0].acc_samples == 0)
        return set_err(ctx, RT_ERR_STATE, "%s: the accumulation has no samples yet", what);
    if (read && !out) return set_err(ctx, RT_ERR_ARG, "output must not be NULL");
    const int64_t npix = ctx->devs[0].acc_npix;
    const int W = (int)ctx->devs[0].acc_cam[6];
    const size_t elem = rgb8 >= 0 ? 1 : sizeof(float);
    // every slot's launch is enqueued before the host waits for any
    for (int k = 0; k < nd; ++k) {
        Device& d = ctx->devs[k];
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, grow(d, d.out, (size_t)d.acc_nloc * 3 * sizeof(float)));
        if (out) HIP_OR_RET(ctx, grow_stage(d, (size_t)d.acc_nloc * 3 * elem));
        if (!read) {
            const int st = selected ? rt_accum_add_selected_device(ctx, k, spp, (float*)d.out.p, d.stream)
                                    : rt_accum_add_device(ctx, k, spp, (float*)d.out.p, d.stream);
            if (st) return st;
        } else if (d.acc_nloc > 0) {
            HIP_OR_RET(ctx, order_after_last(d, d.stream));
            HIP_OR_RET(ctx, rt::launch_accum_resolve((const float4*)d.accum.p, (float*)d.out.p, d.acc_nloc, d.stream));
            HIP_OR_RET(ctx, mark_launch(d, d.stream));
        }
        if (!out || d.acc_nloc == 0) continue;
        const int st = readback_enqueue(ctx, d, d.acc_nloc, rgb8);
        if (st) return st;
    }
    return readback_finish(ctx, out, elem, npix, W);
}
}  // namespace

int rt_accum_begin_device(rt_ctx* ctx, int device_index, const float cam[10], const float env[5], int64_t npix,
                          int max_bounce, int row0, int row_step) {
    rt::FrameParams fp;
    Device* dp = nullptr;
    int st = check_frame(ctx, cam, env, npix, 0, max_bounce, row0, row_step, &fp);
    if (!st) st = slot_of(ctx, device_index, &dp);
    if (st) return st;
    Device& d = *dp;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    d.acc_open = false;   // replaces the slot's accumulation
    d.acc_valid = false;
    d.acc_lens = false;
    d.acc_centre_ready = false;
    HIP_OR_RET(ctx, grow(d, d.accum, (size_t)fp.nloc * 2 * sizeof(float4)));
    std::memcpy(d.acc_cam, cam, sizeof d.acc_cam);
    std::memcpy(d.acc_env, env, sizeof d.acc_env);
    d.acc_npix = npix;
    d.acc_nloc = fp.nloc;
    d.acc_max_bounce = max_bounce;
    d.acc_row0 = row0;
    d.acc_row_step = row_step;
    d.acc_samples = 0;
    accum_reset_selection(d);
    d.acc_open = true;
    d.acc_valid = true;
    ctx->accum_host = false;
    return RT_OK;
}

int rt_accum_add_device(rt_ctx* ctx, int device_index, int spp, float* d_out, void* stream) {
    Device* dp = nullptr;
    int st = slot_of(ctx, device_index, &dp);
    if (!st) st = accum_check_add(ctx, *dp, spp);
    if (st) return st;
    Device& d = *dp;
    rt::FrameParams fp;
    // the frame as begun, at the samples done after this add, under the options as they are now
    st = check_frame(ctx, d.acc_cam, d.acc_env, d.acc_npix, (int)(d.acc_samples + spp), d.acc_max_bounce, d.acc_row0,
                     d.acc_row_step, &fp);
    if (st) return st;
    if (!d_out && fp.nloc > 0) return set_err(ctx, RT_ERR_ARG, "d_out must not be NULL");
    if (d.acc_lens && (st = lens_fits(ctx, dev_scene(ctx, d), "rt_accum_add")) != RT_OK) return st;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    hipStream_t s = (hipStream_t)stream;
    HIP_OR_RET(ctx, order_after_last(d, s));
    if (d.acc_lens) {
        // a lens frame: the tile mapping of the lens loop, every pixel from its record's own count -- so the same
        // launch whether or not the counts differ -- then the frame resolved from the state
        if (fp.nloc > 0) {
            st = accum_add_lens(ctx, d, fp, spp, nullptr, nullptr, s);
            if (st) return st;
            HIP_OR_RET(ctx, rt::launch_accum_resolve((const float4*)d.accum.p, d_out, fp.nloc, s));
            HIP_OR_RET(ctx, mark_launch(d, s));
        }
        d.acc_samples += spp;
        d.acc_full += spp;
        return RT_OK;
    }
    if (!d.acc_uniform && fp.nloc > 0) {
        // the pixels' counts differ (rt_accum_add_selected): the listed kernel over every pixel, each from its own
        // count, then the frame resolved from the state (pixel by pixel the divisor differs)
        HIP_OR_RET(ctx, grow(d, d.all, (size_t)fp.nloc * 4 + 4));
        uint32_t* all = (uint32_t*)d.all.p;
        if (!d.acc_all_ready) HIP_OR_RET(ctx, rt::launch_list_all(all, fp.nloc, all + fp.nloc, s));
        d.acc_all_ready = true;
        fp.spp = spp;
        d.acc_valid = false;
        HIP_OR_RET(ctx, rt::launch_accum_listed(dev_scene(ctx, d), fp, (float4*)d.accum.p, all, all + fp.nloc,
                                                effective_traversal(ctx), ctx->block, d_out, (unsigned int*)d.work.p, s));
        HIP_OR_RET(ctx, rt::launch_accum_resolve((const float4*)d.accum.p, d_out, fp.nloc, s));
        HIP_OR_RET(ctx, mark_launch(d, s));
        d.acc_valid = true;
        d.acc_samples += spp;
        d.acc_full += spp;
        return RT_OK;
    }
    // an add is one pass: no pilot pass and no trails (whatever "pilot" and "spec" say); sample slices as
    // rt_render_device would take them, over the samples this add runs
    HIP_OR_RET(ctx, setup_slices(ctx, d, fp, s, (int)d.acc_samples));
    d.acc_full += spp;
    if (fp.nloc > 0) {
        d.acc_valid = false;   // (an error below leaves the state undefined)
        HIP_OR_RET(ctx, rt::launch_accum(dev_scene(ctx, d), fp, (float4*)d.accum.p, (int)d.acc_samples,
                                         effective_traversal(ctx), ctx->block, d_out, (unsigned int*)d.work.p, s));
        HIP_OR_RET(ctx, mark_launch(d, s));
        d.acc_valid = true;
    }
    d.acc_samples += spp;
    return RT_OK;
}

int rt_accum_begin(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int max_bounce) {
    rt::FrameParams fp;
    int st = check_frame(ctx, cam, env, npix, 0, max_bounce, 0, 1, &fp);
    if (st) return st;
    const int nd = (int)ctx->devs.size();
    for (int k = 0; k < nd; ++k) {
        st = rt_accum_begin_device(ctx, k, cam, env, npix, max_bounce, k, nd);
        if (st) return st;
    }
    ctx->accum_host = true;
    return RT_OK;
}

// A lens accumulation: rt_accum_begin_device's slot, then the lens and the records every add resumes from (the
// initialisation runs on the slot's own stream; launches on other streams are ordered after it like any other)
int rt_accum_begin_lens_device(rt_ctx* ctx, int device_index, const float cam[10], const float env[5],
                               const rt_lens* lens, int64_t npix, int max_bounce, int row0, int row_step) {
    rt::FrameParams fp;
    Device* dp = nullptr;
    int st = check_frame(ctx, cam, env, npix, 0, max_bounce, row0, row_step, &fp);
    if (!st) st = lens_check(ctx, lens);
    if (!st) st = slot_of(ctx, device_index, &dp);
    if (!st) st = lens_fits(ctx, dev_scene(ctx, *dp), "rt_accum_begin_lens");
    if (!st) st = rt_accum_begin_device(ctx, device_index, cam, env, npix, max_bounce, row0, row_step);
    if (st) return st;
    Device& d = *dp;
    d.acc_open = false;   // (until the records are enqueued)
    d.acc_valid = false;
    HIP_OR_RET(ctx, grow(d, d.rad_work, rt::radiance_work_bytes()));
    HIP_OR_RET(ctx, order_after_last(d, d.stream));
    HIP_OR_RET(ctx, rt::launch_lens_accum_init(fp, (float4*)d.accum.p, d.stream));
    HIP_OR_RET(ctx, mark_launch(d, d.stream));
    d.acc_lens = true;
    d.acc_lens_opt = lens_options(lens);
    d.acc_open = true;
    d.acc_valid = true;
    return RT_OK;
}

int rt_accum_begin_lens(rt_ctx* ctx, const float cam[10], const float env[5], const rt_lens* lens, int64_t npix,
                        int max_bounce) {
    rt::FrameParams fp;
    int st = check_frame(ctx, cam, env, npix, 0, max_bounce, 0, 1, &fp);
    if (!st) st = lens_check(ctx, lens);
    if (st) return st;
    const int nd = (int)ctx->devs.size();
    for (int k = 0; k < nd; ++k) {
        st = rt_accum_begin_lens_device(ctx, k, cam, env, lens, npix, max_bounce, k, nd);
        if (st) return st;
    }
    ctx->accum_host = true;
    return RT_OK;
}

int rt_accum_add(rt_ctx* ctx, int spp, float* out_rgb) {
    return accum_host(ctx, spp, false, out_rgb, -1, "rt_accum_add");
}

int rt_accum_add_rgb8(rt_ctx* ctx, int spp, int gamma, uint8_t* out_rgb8) {
    if (ctx && gamma != 0 && gamma != 1) return set_err(ctx, RT_ERR_ARG, "gamma must be 0 or 1");
    return accum_host(ctx, spp, false, out_rgb8, gamma, "rt_accum_add_rgb8");
}

int rt_accum_read(rt_ctx* ctx, float* out_rgb) { return accum_host(ctx, 0, true, out_rgb, -1, "rt_accum_read"); }

int64_t rt_accum_samples(rt_ctx* ctx) {
    if (!ctx) return -1;
    for (const auto& d : ctx->devs)
        if (d.acc_open) return d.acc_samples;
    return -1;
}

int rt_accum_end(rt_ctx* ctx) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    int rc = RT_OK;
    for (auto& d : ctx->devs) {
        const int st = accum_close_slot(ctx, d);
        if (st && !rc) rc = st;
    }
    ctx->accum_host = false;
    return rc;
}

// ---- adaptive sampling: mark, select, add to the selection ----
int rt_accum_mark_device(rt_ctx* ctx, int device_index, void* stream) {
    Device* dp = nullptr;
    const int st = accum_slot_of(ctx, device_index, "rt_accum_mark", &dp);
    if (st) return st;
    Device& d = *dp;
    hipStream_t s = (hipStream_t)stream;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, grow(d, d.mark, (size_t)d.acc_nloc * sizeof(float4)));
    HIP_OR_RET(ctx, order_after_last(d, s));
    d.acc_marked = false;
    HIP_OR_RET(ctx, rt::launch_accum_mark((const float4*)d.accum.p, (float4*)d.mark.p, d.acc_nloc, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    d.acc_marked = true;
    return RT_OK;
}

int rt_accum_select_device(rt_ctx* ctx, int device_index, float threshold, void* stream) {
    Device* dp = nullptr;
    const int st = accum_slot_of(ctx, device_index, "rt_accum_select", &dp);
    if (st) return st;
    if (!dp->acc_marked) return set_err(ctx, RT_ERR_STATE, "rt_accum_select: no mark (rt_accum_mark)");
    return accum_select_slot(ctx, *dp, 0, threshold, nullptr, (hipStream_t)stream);
}

int rt_accum_select_mask_device(rt_ctx* ctx, int device_index, const uint8_t* d_mask, void* stream) {
    Device* dp = nullptr;
    const int st = accum_slot_of(ctx, device_index, "rt_accum_select_mask", &dp);
    if (st) return st;
    if (!d_mask && dp->acc_nloc > 0) return set_err(ctx, RT_ERR_ARG, "rt_accum_select_mask: d_mask must not be NULL");
    return accum_select_slot(ctx, *dp, 1, 0.0f, d_mask, (hipStream_t)stream);
}

int rt_accum_select_all_device(rt_ctx* ctx, int device_index, void* stream) {
    Device* dp = nullptr;
    const int st = accum_slot_of(ctx, device_index, "rt_accum_select_all", &dp);
    if (st) return st;
    return accum_select_slot(ctx, *dp, 2, 0.0f, nullptr, (hipStream_t)stream);
}

int rt_accum_add_selected_device(rt_ctx* ctx, int device_index, int spp, float* d_out, void* stream) {
    Device* dp = nullptr;
    int st = slot_of(ctx, device_index, &dp);
    if (!st) st = accum_check_add_selected(ctx, *dp, spp);
    if (st) return st;
    Device& d = *dp;
    rt::FrameParams fp;
    st = check_frame(ctx, d.acc_cam, d.acc_env, d.acc_npix, spp, d.acc_max_bounce, d.acc_row0, d.acc_row_step, &fp);
    if (st) return st;
    if (!d_out && fp.nloc > 0) return set_err(ctx, RT_ERR_ARG, "d_out must not be NULL");
    if (fp.nloc <= 0) return RT_OK;
    if (d.acc_lens && (st = lens_fits(ctx, dev_scene(ctx, d), "rt_accum_add_selected")) != RT_OK) return st;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    hipStream_t s = (hipStream_t)stream;
    HIP_OR_RET(ctx, order_after_last(d, s));
    if (d.sel_known != 0) {   // (a selection the host knows to be empty adds nothing)
        const SelView v = sel_view(d);
        if (d.acc_lens) {   // the listed mapping of the lens loop over the same list
            st = accum_add_lens(ctx, d, fp, spp, v.list, v.count, s);
            if (st) return st;
        } else {
            d.acc_valid = false;   // (an error below leaves the state undefined)
            HIP_OR_RET(ctx, rt::launch_accum_listed(dev_scene(ctx, d), fp, (float4*)d.accum.p, v.list, v.count,
                                                    effective_traversal(ctx), ctx->block, d_out, (unsigned int*)d.work.p, s));
            d.acc_valid = true;
        }
        d.acc_samples += spp;
        if (!(d.sel_all && d.acc_uniform)) d.acc_uniform = false;
        else d.acc_full += spp;   // (every pixel, all at one count: a full add by another name)
    }
    // the whole frame, every pixel at its own count (the kernel wrote the listed pixels only)
    HIP_OR_RET(ctx, rt::launch_accum_resolve((const float4*)d.accum.p, d_out, d.acc_nloc, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}

int rt_accum_mark(rt_ctx* ctx) {
    const int open = accum_host_open(ctx, "rt_accum_mark");
    if (open) return open;
    for (int k = 0; k < (int)ctx->devs.size(); ++k) {
        const int st = rt_accum_mark_device(ctx, k, ctx->devs[k].stream);
        if (st) return st;
    }
    return RT_OK;
}

int rt_accum_select(rt_ctx* ctx, float threshold, int64_t* n_selected) {
    return accum_select_host(ctx, 0, threshold, nullptr, n_selected, "rt_accum_select");
}

int rt_accum_select_mask(rt_ctx* ctx, const uint8_t* mask) {
    return accum_select_host(ctx, 1, 0.0f, mask, nullptr, "rt_accum_select_mask");
}

int rt_accum_select_all(rt_ctx* ctx) { return accum_select_host(ctx, 2, 0.0f, nullptr, nullptr, "rt_accum_select_all"); }

int rt_accum_selection(rt_ctx* ctx, uint8_t* mask_out) {
    const int open = accum_host_open(ctx, "rt_accum_selection");
    if (open) return open;
    if (!mask_out) return set_err(ctx, RT_ERR_ARG, "mask_out must not be NULL");
    for (const auto& d : ctx->devs) {
        const int st = accum_slot_usable(ctx, d, "rt_accum_selection");
        if (st) return st;
        if (!d.acc_selected) return set_err(ctx, RT_ERR_STATE, "rt_accum_selection: no selection (rt_accum_select*)");
    }
    return accum_gather_host(ctx, mask_out, 1, [](Device& d) { return (const void*)sel_view(d).flag; });
}

int rt_accum_sample_map(rt_ctx* ctx, int32_t* out) {
    const int open = accum_host_open(ctx, "rt_accum_sample_map");
    if (open) return open;
    if (!out) return set_err(ctx, RT_ERR_ARG, "out must not be NULL");
    for (int k = 0; k < (int)ctx->devs.size(); ++k) {
        Device* dp = nullptr;
        const int st = accum_slot_of(ctx, k, "rt_accum_sample_map", &dp);
        if (st) return st;
    }
    for (auto& d : ctx->devs) {   // the counts out of the state, staged in d.out
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, grow(d, d.out, (size_t)d.acc_nloc * sizeof(int32_t)));
        HIP_OR_RET(ctx, order_after_last(d, d.stream));
        HIP_OR_RET(ctx, rt::launch_sample_map((const float4*)d.accum.p, (int32_t*)d.out.p, d.acc_nloc, d.stream));
        HIP_OR_RET(ctx, mark_launch(d, d.stream));
    }
    return accum_gather_host(ctx, out, sizeof(int32_t), [](Device& d) { return (const void*)d.out.p; });
}

int rt_accum_add_selected(rt_ctx* ctx, int spp, float* out_rgb) {
    return accum_host(ctx, spp, false, out_rgb, -1, "rt_accum_add_selected", true);
}

// ---- denoised previews: the guide buffers of the state, the filter ----
namespace {
int denoise_params(rt_ctx* ctx, const rt_denoise_params* in, rt_denoise_params* out) {
    const rt_denoise_params defaults = {5, 5, 1.5f, 0.02f};
    *out = in ? *in : defaults;
    if (out->passes < 1 || out->passes > 8)
        return set_err(ctx, RT_ERR_ARG, "denoise: passes must be 1..8, got %d", out->passes);
    if (out->normal_squarings < 0 || out->normal_squarings > 8)
        return set_err(ctx, RT_ERR_ARG, "denoise: normal_squarings must be 0..8, got %d", out->normal_squarings);
    if (!(std::isfinite(out->sigma_c) && out->sigma_c > 0.0f) || !(std::isfinite(out->sigma_p) && out->sigma_p > 0.0f))
        return set_err(ctx, RT_ERR_ARG, "denoise: sigma_c and sigma_p must be finite and > 0, got %g, %g",
                       (double)out->sigma_c, (double)out->sigma_p);
    return RT_OK;
}

// the open host accumulation, every slot usable and holding samples (the checks of rt_accum_read)
int accum_host_readable(rt_ctx* ctx, const char* what) {
    int st = accum_host_open(ctx, what);
    for (int k = 0; !st && k < (int)ctx->devs.size(); ++k) {
        Device* dp = nullptr;
        st = accum_slot_of(ctx, k, what, &dp);
    }
    return st;
}
}  // namespace

int rt_accum_guides_device(rt_ctx* ctx, int device_index, float* d_guides, void* stream) {
    Device* dp = nullptr;
    int st = accum_slot_of(ctx, device_index, "rt_accum_guides", &dp);
    if (st) return st;
    Device& d = *dp;
    if (!d_guides) return set_err(ctx, RT_ERR_ARG, "rt_accum_guides: the output must not be NULL");
    if ((uintptr_t)d_guides & 15) return set_err(ctx, RT_ERR_ARG, "rt_accum_guides: d_guides must be 16-byte aligned");
    rt::FrameParams fp;
    st = check_frame(ctx, d.acc_cam, d.acc_env, d.acc_npix, 0, d.acc_max_bounce, d.acc_row0, d.acc_row_step, &fp);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    if (d.acc_lens) {
        // a lens record's k, tri are its last sample's hit: the guides' first hit is that of the pixel-centre pinhole
        // ray, traced once per accumulation into d.centre -- the one case in which a guides call traces a ray
        const rt::DevScene sc = dev_scene(ctx, d);
        if (!d.acc_centre_ready && (st = lens_fits(ctx, sc, "rt_accum_guides")) != RT_OK) return st;
        HIP_OR_RET(ctx, grow(d, d.centre, (size_t)d.acc_nloc * sizeof(float2)));
        HIP_OR_RET(ctx, order_after_last(d, s));
        if (!d.acc_centre_ready)
            HIP_OR_RET(ctx, rt::launch_lens_centre(sc, effective_traversal(ctx), fp, (float2*)d.centre.p, d.rad_work.p, s));
        HIP_OR_RET(ctx, rt::launch_lens_guides(sc, fp, (const float4*)d.accum.p, (const float2*)d.centre.p, d.rad_work.p,
                                               (float4*)d_guides, s));
        HIP_OR_RET(ctx, mark_launch(d, s));
        d.acc_centre_ready = true;
        return RT_OK;
    }
    HIP_OR_RET(ctx, grow(d, d.dn_const, rt::launch_const_bytes()));
    HIP_OR_RET(ctx, order_after_last(d, s));
    HIP_OR_RET(ctx, rt::launch_accum_guides(dev_scene(ctx, d), fp, (const float4*)d.accum.p, d.dn_const.p,
                                            (float4*)d_guides, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}

int rt_accum_guides(rt_ctx* ctx, float* out) {
    int st = accum_host_readable(ctx, "rt_accum_guides");
    if (st) return st;
    if (!out) return set_err(ctx, RT_ERR_ARG, "rt_accum_guides: the output must not be NULL");
    for (int k = 0; k < (int)ctx->devs.size(); ++k) {
        Device& d = ctx->devs[k];
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, grow(d, d.guides, (size_t)d.acc_nloc * 12 * sizeof(float)));
        st = rt_accum_guides_device(ctx, k, (float*)d.guides.p, d.stream);
        if (st) return st;
    }
    return accum_gather_host(ctx, out, 12 * sizeof(float), [](Device& d) { return (const void*)d.guides.p; });
}

int rt_denoise_device(rt_ctx* ctx, int device_index, const float* d_rgb, const float* d_guides, int64_t npix, int width,
                      const rt_denoise_params* params, float* d_out, void* stream) {
    Device* dp = nullptr;
    rt_denoise_params P;
    int st = slot_of(ctx, device_index, &dp);
    if (!st) st = denoise_params(ctx, params, &P);
    if (st) return st;
    if (!d_rgb || !d_guides || !d_out) return set_err(ctx, RT_ERR_ARG, "rt_denoise_device: NULL buffer");
    if ((uintptr_t)d_guides & 15) return set_err(ctx, RT_ERR_ARG, "rt_denoise_device: d_guides must be 16-byte aligned");
    if (npix < 1 || npix > 0x7fffffff || width < 1)
        return set_err(ctx, RT_ERR_ARG, "rt_denoise_device: bad frame (%lld pixels, rows of %d)", (long long)npix, width);
    Device& d = *dp;
    hipStream_t s = (hipStream_t)stream;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, grow(d, d.dn, rt::denoise_scratch_bytes(npix)));
    HIP_OR_RET(ctx, order_after_last(d, s));
    HIP_OR_RET(ctx, rt::launch_denoise(d_rgb, (const float4*)d_guides, npix, width, P.passes, P.normal_squarings,
                                       P.sigma_c, P.sigma_p, (ctx->denoise_lds >= 0 ? ctx->denoise_lds : kDenoiseLds) != 0,
                                       (float4*)d.dn.p, d_out, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}

namespace {
// The open host accumulation's frame and guides in frame order on slot 0 (the checks of accum_host_readable are the
// caller's): every slot resolves the rows it holds; one slot: its tile is the frame, everything stays on the device;
// several: the rows are assembled into frame-shaped buffers on slot 0, through the host.  Enqueued on slot 0's stream.
int accum_frame_on_slot0(rt_ctx* ctx, const float** rgb_out, const float** guides_out) {
    const int nd = (int)ctx->devs.size();
    const int64_t npix = ctx->devs[0].acc_npix;
    for (int k = 0; k < nd; ++k) {
        Device& d = ctx->devs[k];
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, grow(d, d.out, (size_t)d.acc_nloc * 3 * sizeof(float)));
        HIP_OR_RET(ctx, grow(d, d.guides, (size_t)d.acc_nloc * 12 * sizeof(float)));
        if (d.acc_nloc > 0) {
            HIP_OR_RET(ctx, order_after_last(d, d.stream));
            HIP_OR_RET(ctx, rt::launch_accum_resolve((const float4*)d.accum.p, (float*)d.out.p, d.acc_nloc, d.stream));
            HIP_OR_RET(ctx, mark_launch(d, d.stream));
        }
        const int st = rt_accum_guides_device(ctx, k, (float*)d.guides.p, d.stream);
        if (st) return st;
    }
    Device& d0 = ctx->devs[0];
    *rgb_out = (const float*)d0.out.p;
    *guides_out = (const float*)d0.guides.p;
    if (nd > 1) {
        std::vector<float> h_rgb((size_t)npix * 3), h_guides((size_t)npix * 12);   // (kept until the uploads are done)
        int st = accum_gather_host(ctx, h_rgb.data(), 3 * sizeof(float), [](Device& d) { return (const void*)d.out.p; });
        if (st) return st;
        st = accum_gather_host(ctx, h_guides.data(), 12 * sizeof(float), [](Device& d) { return (const void*)d.guides.p; });
        if (st) return st;
        HIP_OR_RET(ctx, hipSetDevice(d0.id));
        HIP_OR_RET(ctx, grow(d0, d0.dn_rgb, h_rgb.size() * sizeof(float)));
        HIP_OR_RET(ctx, grow(d0, d0.dn_guides, h_guides.size() * sizeof(float)));
        HIP_OR_RET(ctx, order_after_last(d0, d0.stream));
        HIP_OR_RET(ctx, hipMemcpyAsync(d0.dn_rgb.p, h_rgb.data(), h_rgb.size() * sizeof(float), hipMemcpyHostToDevice, d0.stream));
        HIP_OR_RET(ctx, hipMemcpyAsync(d0.dn_guides.p, h_guides.data(), h_guides.size() * sizeof(float), hipMemcpyHostToDevice,
                                       d0.stream));
        HIP_OR_RET(ctx, hipStreamSynchronize(d0.stream));
        *rgb_out = (const float*)d0.dn_rgb.p;
        *guides_out = (const float*)d0.dn_guides.p;
    }
    return RT_OK;
}
}  // namespace

int rt_accum_denoise(rt_ctx* ctx, const rt_denoise_params* params, float* out_rgb) {
    int st = accum_host_readable(ctx, "rt_accum_denoise");
    if (st) return st;
    if (!out_rgb) return set_err(ctx, RT_ERR_ARG, "rt_accum_denoise: the output must not be NULL");
    rt_denoise_params P;
    st = denoise_params(ctx, params, &P);
    if (st) return st;
    const int64_t npix = ctx->devs[0].acc_npix;
    const int W = (int)ctx->devs[0].acc_cam[6];
    const float *rgb, *guides;
    st = accum_frame_on_slot0(ctx, &rgb, &guides);
    if (st) return st;
    Device& d0 = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d0.id));
    HIP_OR_RET(ctx, grow(d0, d0.dn_out, (size_t)npix * 3 * sizeof(float)));
    st = rt_denoise_device(ctx, 0, rgb, guides, npix, W, &P, (float*)d0.dn_out.p, d0.stream);
    if (st) return st;
    HIP_OR_RET(ctx, hipMemcpyAsync(out_rgb, d0.dn_out.p, (size_t)npix * 3 * sizeof(float), hipMemcpyDeviceToHost, d0.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d0.stream));
    return RT_OK;
}

int rt_denoise(rt_ctx* ctx, const float* rgb, const float* guides, int64_t npix, int width,
               const rt_denoise_params* params, float* out_rgb) {
    Device* dp = nullptr;
    rt_denoise_params P;
    int st = slot_of(ctx, 0, &dp);
    if (!st) st = denoise_params(ctx, params, &P);
    if (st) return st;
    if (!rgb || !guides || !out_rgb) return set_err(ctx, RT_ERR_ARG, "rt_denoise: NULL buffer");
    if (npix < 1 || npix > 0x7fffffff || width < 1)
        return set_err(ctx, RT_ERR_ARG, "rt_denoise: bad frame (%lld pixels, rows of %d)", (long long)npix, width);
    Device& d = *dp;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, grow(d, d.rp_rgb, (size_t)npix * 3 * sizeof(float)));
    HIP_OR_RET(ctx, grow(d, d.rp_guides, (size_t)npix * 12 * sizeof(float)));
    HIP_OR_RET(ctx, grow(d, d.dn_out, (size_t)npix * 3 * sizeof(float)));
    HIP_OR_RET(ctx, order_after_last(d, d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(d.rp_rgb.p, rgb, (size_t)npix * 3 * sizeof(float), hipMemcpyHostToDevice, d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(d.rp_guides.p, guides, (size_t)npix * 12 * sizeof(float), hipMemcpyHostToDevice, d.stream));
    st = rt_denoise_device(ctx, 0, (const float*)d.rp_rgb.p, (const float*)d.rp_guides.p, npix, width, &P,
                           (float*)d.dn_out.p, d.stream);
    if (st) return st;
    HIP_OR_RET(ctx, hipMemcpyAsync(out_rgb, d.dn_out.p, (size_t)npix * 3 * sizeof(float), hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

// ---- temporal reprojection: the previous frame and guides gathered into the current view ----
namespace {
int reproject_params(rt_ctx* ctx, const rt_reproject_params* in, rt::ReprojectParams* out) {
    const rt_reproject_params defaults = {0.02f, 0.9f, 64.0f, 0.25f};
    const rt_reproject_params p = in ? *in : defaults;
    if (!(std::isfinite(p.sigma_p) && p.sigma_p > 0.0f) || !(std::isfinite(p.max_history) && p.max_history > 0.0f))
        return set_err(ctx, RT_ERR_ARG, "reproject: sigma_p and max_history must be finite and > 0, got %g, %g",
                       (double)p.sigma_p, (double)p.max_history);
    if (!std::isfinite(p.normal_min) || !std::isfinite(p.min_weight))
        return set_err(ctx, RT_ERR_ARG, "reproject: normal_min and min_weight must be finite, got %g, %g",
                       (double)p.normal_min, (double)p.min_weight);
    *out = rt::ReprojectParams{p.sigma_p, p.normal_min, p.max_history, p.min_weight};
    return RT_OK;
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}
}  // namespace

int rt_reproject_device(rt_ctx* ctx, int device_index, const float* d_prev_rgb, const float* d_prev_guides,
                        const float prev_cam[10], const float* d_cur_rgb, const float* d_cur_guides, int64_t npix,
                        int width, const rt_reproject_params* params, float* d_out_rgb, float* d_out_guides,
                        void* stream) {
    Device* dp = nullptr;
    rt::ReprojectParams P;
    int st = slot_of(ctx, device_index, &dp);
    if (!st) st = reproject_params(ctx, params, &P);
    if (st) return st;
    if (!d_prev_rgb || !d_prev_guides || !prev_cam || !d_cur_rgb || !d_cur_guides || !d_out_rgb || !d_out_guides)
        return set_err(ctx, RT_ERR_ARG, "rt_reproject_device: NULL buffer");
    if (npix < 1 || npix > 0x7fffffff || width < 1)
        return set_err(ctx, RT_ERR_ARG, "rt_reproject_device: bad frame (%lld pixels, rows of %d)", (long long)npix, width);
    float basis[16];
    if (rt_reproject_basis(prev_cam, basis) != RT_OK)
        return set_err(ctx, RT_ERR_ARG, "rt_reproject_device: prev_cam must be finite");
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(basis[k])) return set_err(ctx, RT_ERR_ARG, "rt_reproject_device: prev_cam has no finite basis");
    if ((int)prev_cam[6] != width)
        return set_err(ctx, RT_ERR_ARG, "rt_reproject_device: prev_cam's width %d is not the frame's %d", (int)prev_cam[6],
                       width);
    if (((uintptr_t)d_prev_guides & 15) || ((uintptr_t)d_cur_guides & 15) || ((uintptr_t)d_out_guides & 15))
        return set_err(ctx, RT_ERR_ARG, "rt_reproject_device: the guides must be 16-byte aligned");
    const size_t nrgb = (size_t)npix * 3 * sizeof(float), ng = (size_t)npix * 12 * sizeof(float);
    const struct { const void* p; size_t n; } ins[4] = {{d_prev_rgb, nrgb}, {d_prev_guides, ng}, {d_cur_rgb, nrgb},
                                                         {d_cur_guides, ng}};
    bool overlap = ranges_overlap(d_out_rgb, nrgb, d_out_guides, ng);
    for (const auto& in : ins)
        overlap = overlap || ranges_overlap(d_out_rgb, nrgb, in.p, in.n) || ranges_overlap(d_out_guides, ng, in.p, in.n);
    if (overlap) return set_err(ctx, RT_ERR_ARG, "rt_reproject_device: the outputs overlap an input or each other");
    rt::ReprojectBasis B;
    std::memcpy(B.m, basis, sizeof(B.m));
    std::memcpy(B.pos, basis + 9, sizeof(B.pos));
    B.f = basis[12];
    B.cam6 = basis[13];
    Device& d = *dp;
    hipStream_t s = (hipStream_t)stream;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, order_after_last(d, s));
    HIP_OR_RET(ctx, rt::launch_reproject(d_prev_rgb, (const float4*)d_prev_guides, d_cur_rgb, (const float4*)d_cur_guides,
                                         npix, width, B, P, d_out_rgb, (float4*)d_out_guides, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}

int rt_accum_reproject(rt_ctx* ctx, const float* prev_rgb, const float* prev_guides, const float prev_cam[10],
                       const rt_reproject_params* params, float* out_rgb, float* out_guides) {
    int st = accum_host_readable(ctx, "rt_accum_reproject");
    if (st) return st;
    if (!prev_rgb || !prev_guides || !prev_cam || !out_rgb || !out_guides)
        return set_err(ctx, RT_ERR_ARG, "rt_accum_reproject: NULL buffer");
    rt::ReprojectParams P;
    st = reproject_params(ctx, params, &P);
    if (st) return st;
    const int64_t npix = ctx->devs[0].acc_npix;
    const int W = (int)ctx->devs[0].acc_cam[6];
    float basis[16];
    if (rt_reproject_basis(prev_cam, basis) != RT_OK || (int)prev_cam[6] != W)   // (before anything is enqueued)
        return set_err(ctx, RT_ERR_ARG, "rt_accum_reproject: prev_cam must be finite and of the accumulation's width %d", W);
    const float *rgb, *guides;
    st = accum_frame_on_slot0(ctx, &rgb, &guides);
    if (st) return st;
    Device& d0 = ctx->devs[0];
    const size_t nrgb = (size_t)npix * 3 * sizeof(float), ng = (size_t)npix * 12 * sizeof(float);
    HIP_OR_RET(ctx, hipSetDevice(d0.id));
    HIP_OR_RET(ctx, grow(d0, d0.rp_rgb, nrgb));
    HIP_OR_RET(ctx, grow(d0, d0.rp_guides, ng));
    HIP_OR_RET(ctx, grow(d0, d0.dn_out, nrgb));
    HIP_OR_RET(ctx, grow(d0, d0.rp_out_guides, ng));
    HIP_OR_RET(ctx, order_after_last(d0, d0.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(d0.rp_rgb.p, prev_rgb, nrgb, hipMemcpyHostToDevice, d0.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(d0.rp_guides.p, prev_guides, ng, hipMemcpyHostToDevice, d0.stream));
    st = rt_reproject_device(ctx, 0, (const float*)d0.rp_rgb.p, (const float*)d0.rp_guides.p, prev_cam, rgb, guides, npix, W,
                             params, (float*)d0.dn_out.p, (float*)d0.rp_out_guides.p, d0.stream);
    if (st) return st;
    HIP_OR_RET(ctx, hipMemcpyAsync(out_rgb, d0.dn_out.p, nrgb, hipMemcpyDeviceToHost, d0.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(out_guides, d0.rp_out_guides.p, ng, hipMemcpyDeviceToHost, d0.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d0.stream));
    return RT_OK;
}

int rt_render(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp, int max_bounce,
              float* out_rgb) {
    return render_host(ctx, cam, env, npix, spp, max_bounce, out_rgb, -1);
}

int rt_render_rgb8(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp, int max_bounce,
                   int gamma, uint8_t* out_rgb8) {
    if (ctx && gamma != 0 && gamma != 1) return set_err(ctx, RT_ERR_ARG, "gamma must be 0 or 1");
    return render_host(ctx, cam, env, npix, spp, max_bounce, out_rgb8, gamma);
}

int rt_rgb8_device(rt_ctx* ctx, int device_index, const float* d_in, uint8_t* d_out, int64_t n, int gamma,
                   void* stream) {
    Device* dp = nullptr;
    const int st = slot_of(ctx, device_index, &dp, "device_index");
    if (st) return st;
    if (n < 0 || (n > 0 && (!d_in || !d_out)) || (gamma != 0 && gamma != 1))
        return set_err(ctx, RT_ERR_ARG, "bad arguments");
    if (((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 3))
        return set_err(ctx, RT_ERR_ARG, "d_in must be 16-byte and d_out 4-byte aligned");
    HIP_OR_RET(ctx, hipSetDevice(dp->id));
    HIP_OR_RET(ctx, rt::launch_rgb8(d_in, d_out, n, gamma == 1, (hipStream_t)stream));
    return RT_OK;
}

int rt_rgb8(rt_ctx* ctx, const float* in, uint8_t* out, int64_t n, int gamma) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (n < 0 || (n > 0 && (!in || !out)) || (gamma != 0 && gamma != 1))
        return set_err(ctx, RT_ERR_ARG, "bad arguments");
    if (n == 0) return RT_OK;
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, grow(d, d.scratch_a, (size_t)n * sizeof(float)));
    HIP_OR_RET(ctx, grow(d, d.scratch_b, (size_t)n));
    HIP_OR_RET(ctx, hipMemcpyAsync(d.scratch_a.p, in, (size_t)n * sizeof(float), hipMemcpyHostToDevice, d.stream));
    HIP_OR_RET(ctx, rt::launch_rgb8((const float*)d.scratch_a.p, (uint8_t*)d.scratch_b.p, n, gamma == 1, d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(out, d.scratch_b.p, (size_t)n, hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

namespace {
// the refill counters of the last instrumented launch (rt_debug_last_refill)
std::atomic<long long> g_refill_events{0}, g_refill_lanes{0};
int count_all(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp, int max_bounce, int row0,
              int row_step, uint64_t* counts, int n) {
    rt::FrameParams fp;
    int st = check_frame(ctx, cam, env, npix, spp, max_bounce, row0, row_step, &fp);
    if (st) return st;
    if (!counts) return set_err(ctx, RT_ERR_ARG, "counts must not be NULL");
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    const size_t bytes = (size_t)fp.nloc * 3 * sizeof(float);
    HIP_OR_RET(ctx, grow(d, d.out, bytes));
    unsigned long long h[18] = {0};   // the kernels' counters (rt_device.h NCOUNTS), then render_kernel's refill events [15] and lanes refilled [16]
    HIP_OR_RET(ctx, grow(d, d.counts, sizeof h));
    HIP_OR_RET(ctx, hipMemsetAsync(d.counts.p, 0, sizeof h, d.stream));
    HIP_OR_RET(ctx, order_after_last(d, d.stream));
    // the instrumented brute-force launch takes sample slices as the product launch does (the tree walk's
    // counts are those of its unsliced frame)
    if (ctx->hs.nbrute > 0) HIP_OR_RET(ctx, setup_slices(ctx, d, fp, d.stream));
    HIP_OR_RET(ctx, rt::launch_render(dev_scene(ctx, d), fp, effective_traversal(ctx), ctx->block, (float*)d.out.p,
                                      (unsigned long long*)d.counts.p, (unsigned int*)d.work.p, d.stream, nullptr,
                                      &d.pilot_note));
    HIP_OR_RET(ctx, mark_launch(d, d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(h, d.counts.p, sizeof h, hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    for (int q = 0; q < n; ++q) counts[q] = h[q];
    g_refill_lanes.store((long long)h[16], std::memory_order_relaxed);   // (rt_debug_last_refill; h[15] = the events)
    g_refill_events.store((long long)h[15], std::memory_order_relaxed);
    return RT_OK;
}
}  // namespace

int rt_count_work(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp, int max_bounce,
                  int row0, int row_step, uint64_t counts[5]) {
    return count_all(ctx, cam, env, npix, spp, max_bounce, row0, row_step, counts, 5);
}

int rt_count_work_detail(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp, int max_bounce,
                         int row0, int row_step, uint64_t counts[16]) {
    return count_all(ctx, cam, env, npix, spp, max_bounce, row0, row_step, counts, 16);
}

int rt_debug_wave_counts(rt_ctx* ctx, const float cam[10], const float env[5], int64_t npix, int spp, int max_bounce,
                         uint64_t counts[9]) {
    return count_all(ctx, cam, env, npix, spp, max_bounce, 0, 1, counts, 9);
}

int rt_work_bytes(rt_ctx* ctx, double out[4]) {
    // Algorithmic bytes per unit: 32 B per box test (24 B AABB + 8 B child/leaf
    // refs), 36 B per triangle test (v0, e1, e2), 40 B per hit record, 16 B per IBL lookup.
    if (!ctx || !out) return set_err(ctx, RT_ERR_ARG, "null argument");
    // out[0] prices counts[9] (box tests) of rt_count_work_detail: a BVH2 node tests 2 child boxes, a
    // 4-wide node up to 4, a wide leaf its exact box again, a REF node 1 -- so every layout is priced
    // per box actually tested
    out[0] = 32.0;
    out[1] = 36.0;
    out[2] = 40.0;
    out[3] = 16.0;
    return RT_OK;
}

int rt_gamma(rt_ctx* ctx, const float* in, float* out, int64_t n) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (n < 0 || (n > 0 && (!in || !out))) return set_err(ctx, RT_ERR_ARG, "bad arguments");
    if (n == 0) return RT_OK;
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    const size_t bytes = (size_t)n * sizeof(float);
    HIP_OR_RET(ctx, grow(d, d.scratch_a, bytes));
    HIP_OR_RET(ctx, grow(d, d.scratch_b, bytes));
    HIP_OR_RET(ctx, hipMemcpyAsync(d.scratch_a.p, in, bytes, hipMemcpyHostToDevice, d.stream));
    HIP_OR_RET(ctx, rt::launch_gamma((const float*)d.scratch_a.p, (float*)d.scratch_b.p, n, d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(out, d.scratch_b.p, bytes, hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

namespace {
// the argument and state checks the two query entry points share (n > 0 past them)
int query_check(rt_ctx* ctx, const void* rays, int64_t n, int mode, const void* out) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (n < 0 || n >= ((int64_t)1 << 31)) return set_err(ctx, RT_ERR_ARG, "ray count %lld out of range", (long long)n);
    if (mode != RT_QUERY_CLOSEST && mode != RT_QUERY_ANY) return set_err(ctx, RT_ERR_ARG, "no query mode %d", mode);
    if (n > 0 && (!rays || !out)) return set_err(ctx, RT_ERR_ARG, "rays / out must not be NULL");
    if (!ctx->have_scene) return set_err(ctx, RT_ERR_STATE, "rt_set_scene has not been called");
    if (ctx->traversal == RT_TRAVERSAL_FAST && !ctx->hs.fast_ok)
        return set_err(ctx, RT_ERR_STATE, "FAST traversal unavailable for this scene");
    return RT_OK;
}

// one slot's launch: ordered with the context's other launches, never waits
int query_enqueue(rt_ctx* ctx, Device& d, const float* d_rays, int64_t n, int mode, rt_hit* d_out, hipStream_t s) {
    HIP_OR_RET(ctx, grow(d, d.q_counter, 256));
    const rt::QueryOptions q{ctx->query_engine, ctx->query_grid, resume_min_of(ctx), ctx->max_waves, ctx->block};
    HIP_OR_RET(ctx, order_after_last(d, s));
    HIP_OR_RET(ctx, rt::launch_query(dev_scene(ctx, d), ctx->traversal, mode == RT_QUERY_ANY, (const float4*)d_rays,
                                     (float4*)d_out, n, q, (unsigned int*)d.q_counter.p, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}
}  // namespace

int rt_trace_device(rt_ctx* ctx, int device_index, const float* d_rays, int64_t n, int mode, rt_hit* d_out,
                    void* stream) {
    Device* dp = nullptr;
    int st = query_check(ctx, d_rays, n, mode, d_out);
    if (!st) st = slot_of(ctx, device_index, &dp);
    if (st) return st;
    if (n == 0) return RT_OK;
    const uintptr_t r0 = (uintptr_t)d_rays, o0 = (uintptr_t)d_out;
    if ((r0 & 15) || (o0 & 15)) return set_err(ctx, RT_ERR_ARG, "d_rays and d_out must be 16-byte aligned");
    if (r0 < o0 + (uintptr_t)n * sizeof(rt_hit) && o0 < r0 + (uintptr_t)n * 32)
        return set_err(ctx, RT_ERR_ARG, "d_rays and d_out must not overlap");
    HIP_OR_RET(ctx, hipSetDevice(dp->id));
    return query_enqueue(ctx, *dp, d_rays, n, mode, d_out, (hipStream_t)stream);
}

int rt_trace(rt_ctx* ctx, const float* rays, int64_t n, int mode, rt_hit* out) {
    const int st = query_check(ctx, rays, n, mode, out);
    if (st) return st;
    if (n == 0) return RT_OK;
    // contiguous chunks over the slots; every slot is enqueued before any is waited for
    const int64_t nd = (int64_t)ctx->devs.size();
    for (int64_t k = 0; k < nd; ++k) {
        const int64_t b = n * k / nd, m = n * (k + 1) / nd - b;
        if (m <= 0) continue;
        Device& d = ctx->devs[k];
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, grow(d, d.q_rays, (size_t)m * 32));
        HIP_OR_RET(ctx, grow(d, d.q_out, (size_t)m * sizeof(rt_hit)));
        HIP_OR_RET(ctx, hipMemcpyAsync(d.q_rays.p, rays + 8 * b, (size_t)m * 32, hipMemcpyHostToDevice, d.stream));
        const int qs = query_enqueue(ctx, d, (const float*)d.q_rays.p, m, mode, (rt_hit*)d.q_out.p, d.stream);
        if (qs) return qs;
        HIP_OR_RET(ctx, hipMemcpyAsync(out + b, d.q_out.p, (size_t)m * sizeof(rt_hit), hipMemcpyDeviceToHost, d.stream));
    }
    for (auto& d : ctx->devs) {
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    }
    return RT_OK;
}

static_assert(sizeof(rt_radiance_state) == 32, "rt_radiance_state is the accumulation's state record: two float4");
namespace {
// the argument and state checks the two radiance entry points share (n > 0 past them)
int radiance_check(rt_ctx* ctx, const void* rays, int64_t n, const float* env, int spp, int max_bounce, int flags,
                   const void* state) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (n < 0 || n >= ((int64_t)1 << 31)) return set_err(ctx, RT_ERR_ARG, "ray count %lld out of range", (long long)n);
    if (spp < 1 || spp > RT_ACCUM_MAX_SAMPLES) return set_err(ctx, RT_ERR_ARG, "spp %d outside 1..%d", spp, RT_ACCUM_MAX_SAMPLES);
    if (flags & ~RT_RADIANCE_RESUME) return set_err(ctx, RT_ERR_ARG, "unknown flag bits 0x%x", (unsigned)flags);
    if (max_bounce > 4096) return set_err(ctx, RT_ERR_ARG, "maxBounce %d > 4096", max_bounce);
    if (!env) return set_err(ctx, RT_ERR_ARG, "env must not be NULL");
    if (n > 0 && (!rays || !state)) return set_err(ctx, RT_ERR_ARG, "rays / state must not be NULL");
    if (!ctx->have_scene) return set_err(ctx, RT_ERR_STATE, "rt_set_scene has not been called");
    if (!ctx->have_env) return set_err(ctx, RT_ERR_STATE, "rt_set_env has not been called");
    if (ctx->traversal == RT_TRAVERSAL_FAST && !ctx->hs.fast_ok)
        return set_err(ctx, RT_ERR_STATE, "FAST traversal unavailable for this scene");
    return RT_OK;
}

// one slot's launch: ordered with the context's other launches, never waits
int radiance_enqueue(rt_ctx* ctx, Device& d, const float* d_rays, int64_t n, const float env[5], int spp,
                     int max_bounce, int flags, rt_radiance_state* d_state, hipStream_t s) {
    const rt::DevScene sc = dev_scene(ctx, d);
    if (!rt::radiance_fits(sc, ctx->traversal, ctx->block))
        return set_err(ctx, RT_ERR_SCENE, "a traversal stack of %d entries per lane does not fit a block of 64 lanes",
                       ctx->traversal == RT_TRAVERSAL_REF ? (int)sc.ref_stack : (int)sc.depth);
    HIP_OR_RET(ctx, grow(d, d.rad_work, rt::radiance_work_bytes()));
    const rt::RadianceOptions q = radiance_options(ctx, env, spp, max_bounce, flags);
    HIP_OR_RET(ctx, order_after_last(d, s));
    HIP_OR_RET(ctx, rt::launch_radiance(sc, ctx->traversal, (const float4*)d_rays, (float4*)d_state, n, q, d.rad_work.p, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}

int camera_rays_check(rt_ctx* ctx, const float* cam, int64_t npix, int64_t first, int64_t count, const void* rays) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (!cam) return set_err(ctx, RT_ERR_ARG, "cam must not be NULL");
    if (!(cam[6] >= 1.0f) || !(cam[6] < 2147483648.0f))
        return set_err(ctx, RT_ERR_ARG, "cam[6] (row width) must be >= 1, got %g", (double)cam[6]);
    if (npix <= 0 || npix > 0x7fffffff) return set_err(ctx, RT_ERR_ARG, "pixel count %lld out of range", (long long)npix);
    if (first < 0 || count < 0 || first > npix || count > npix - first)
        return set_err(ctx, RT_ERR_ARG, "pixels %lld .. +%lld outside the frame of %lld", (long long)first,
                       (long long)count, (long long)npix);
    if (count > 0 && !rays) return set_err(ctx, RT_ERR_ARG, "rays must not be NULL");
    return RT_OK;
}

int camera_rays_enqueue(rt_ctx* ctx, Device& d, const float cam[10], int64_t npix, int64_t first, int64_t count,
                        float* d_rays, hipStream_t s) {
    HIP_OR_RET(ctx, grow(d, d.rad_work, rt::radiance_work_bytes()));
    HIP_OR_RET(ctx, order_after_last(d, s));
    HIP_OR_RET(ctx, rt::launch_camera_rays(cam, npix, first, count, (float4*)d_rays, d.rad_work.p, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}
}  // namespace

int rt_radiance_device(rt_ctx* ctx, int device_index, const float* d_rays, int64_t n, const float env[5], int spp,
                       int max_bounce, int flags, rt_radiance_state* d_state, void* stream) {
    Device* dp = nullptr;
    int st = radiance_check(ctx, d_rays, n, env, spp, max_bounce, flags, d_state);
    if (!st) st = slot_of(ctx, device_index, &dp);
    if (st) return st;
    if (n == 0) return RT_OK;
    const uintptr_t r0 = (uintptr_t)d_rays, o0 = (uintptr_t)d_state;
    if ((r0 & 15) || (o0 & 15)) return set_err(ctx, RT_ERR_ARG, "d_rays and d_state must be 16-byte aligned");
    if (r0 < o0 + (uintptr_t)n * sizeof(rt_radiance_state) && o0 < r0 + (uintptr_t)n * 32)
        return set_err(ctx, RT_ERR_ARG, "d_rays and d_state must not overlap");
    HIP_OR_RET(ctx, hipSetDevice(dp->id));
    return radiance_enqueue(ctx, *dp, d_rays, n, env, spp, max_bounce, flags, d_state, (hipStream_t)stream);
}

int rt_radiance(rt_ctx* ctx, const float* rays, int64_t n, const float env[5], int spp, int max_bounce, int flags,
                rt_radiance_state* state) {
    const int st = radiance_check(ctx, rays, n, env, spp, max_bounce, flags, state);
    if (st) return st;
    if (n == 0) return RT_OK;
    // contiguous chunks over the slots; every slot is enqueued before any is waited for
    const int64_t nd = (int64_t)ctx->devs.size();
    for (int64_t k = 0; k < nd; ++k) {
        const int64_t b = n * k / nd, m = n * (k + 1) / nd - b;
        if (m <= 0) continue;
        Device& d = ctx->devs[k];
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, grow(d, d.q_rays, (size_t)m * 32));
        HIP_OR_RET(ctx, grow(d, d.rad_state, (size_t)m * sizeof(rt_radiance_state)));
        HIP_OR_RET(ctx, hipMemcpyAsync(d.q_rays.p, rays + 8 * b, (size_t)m * 32, hipMemcpyHostToDevice, d.stream));
        if (flags & RT_RADIANCE_RESUME)
            HIP_OR_RET(ctx, hipMemcpyAsync(d.rad_state.p, state + b, (size_t)m * sizeof(rt_radiance_state),
                                           hipMemcpyHostToDevice, d.stream));
        const int qs = radiance_enqueue(ctx, d, (const float*)d.q_rays.p, m, env, spp, max_bounce, flags,
                                        (rt_radiance_state*)d.rad_state.p, d.stream);
        if (qs) return qs;
        HIP_OR_RET(ctx, hipMemcpyAsync(state + b, d.rad_state.p, (size_t)m * sizeof(rt_radiance_state),
                                       hipMemcpyDeviceToHost, d.stream));
    }
    for (auto& d : ctx->devs) {
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    }
    return RT_OK;
}

int rt_camera_rays_device(rt_ctx* ctx, int device_index, const float cam[10], int64_t npix, int64_t first,
                          int64_t count, float* d_rays, void* stream) {
    Device* dp = nullptr;
    int st = camera_rays_check(ctx, cam, npix, first, count, d_rays);
    if (!st) st = slot_of(ctx, device_index, &dp);
    if (st) return st;
    if (count == 0) return RT_OK;
    if ((uintptr_t)d_rays & 15) return set_err(ctx, RT_ERR_ARG, "d_rays must be 16-byte aligned");
    HIP_OR_RET(ctx, hipSetDevice(dp->id));
    return camera_rays_enqueue(ctx, *dp, cam, npix, first, count, d_rays, (hipStream_t)stream);
}

int rt_camera_rays(rt_ctx* ctx, const float cam[10], int64_t npix, int64_t first, int64_t count, float* rays) {
    const int st = camera_rays_check(ctx, cam, npix, first, count, rays);
    if (st) return st;
    if (count == 0) return RT_OK;
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, grow(d, d.q_rays, (size_t)count * 32));
    const int qs = camera_rays_enqueue(ctx, d, cam, npix, first, count, (float*)d.q_rays.p, d.stream);
    if (qs) return qs;
    HIP_OR_RET(ctx, hipMemcpyAsync(rays, d.q_rays.p, (size_t)count * 32, hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

// ---- lens frames (rt_lens_radiance*, rt_lens_rays*, rt_radiance_resolve_device) ----
static_assert(sizeof(rt_lens) == 16, "rt_lens is four 32-bit words");
namespace {
// the lens, beside camera_rays_check's camera and pixel range
int lens_check(rt_ctx* ctx, const rt_lens* lens) {
    if (!lens) return set_err(ctx, RT_ERR_ARG, "lens must not be NULL");
    if (!std::isfinite(lens->jitter) || lens->jitter < 0.0f)
        return set_err(ctx, RT_ERR_ARG, "lens jitter must be finite and >= 0, got %g", (double)lens->jitter);
    if (!std::isfinite(lens->aperture) || lens->aperture < 0.0f)
        return set_err(ctx, RT_ERR_ARG, "lens aperture must be finite and >= 0, got %g", (double)lens->aperture);
    if (!std::isfinite(lens->focus) || !(lens->focus > 0.0f))
        return set_err(ctx, RT_ERR_ARG, "lens focus must be finite and > 0, got %g", (double)lens->focus);
    return RT_OK;
}

rt::LensOptions lens_options(const rt_lens* lens) {
    rt::LensOptions o;
    o.jitter = lens->jitter;
    o.aperture = lens->aperture;
    o.focus = lens->focus;
    o.seed = lens->seed;
    return o;
}

// the checks the two lens render entry points share: rt_camera_rays' on the camera and the pixels, the lens, then
// rt_radiance's on the rest (whose ray array is the state here: there is none to pass)
int lens_radiance_check(rt_ctx* ctx, const float* cam, const float* env, const rt_lens* lens, int64_t npix,
                        int64_t first, int64_t count, int spp, int max_bounce, int flags, const void* state) {
    int st = camera_rays_check(ctx, cam, npix, first, count, cam);   // (a NULL state is radiance_check's to report)
    if (!st) st = lens_check(ctx, lens);
    if (!st) st = radiance_check(ctx, state, count, env, spp, max_bounce, flags, state);
    return st;
}

int lens_radiance_enqueue(rt_ctx* ctx, Device& d, const float cam[10], const float env[5], const rt_lens* lens,
                          int64_t npix, int64_t first, int64_t count, int spp, int max_bounce, int flags,
                          rt_radiance_state* d_state, hipStream_t s) {
    const rt::DevScene sc = dev_scene(ctx, d);
    if (!rt::radiance_fits(sc, ctx->traversal, ctx->block))
        return set_err(ctx, RT_ERR_SCENE, "a traversal stack of %d entries per lane does not fit a block of 64 lanes",
                       ctx->traversal == RT_TRAVERSAL_REF ? (int)sc.ref_stack : (int)sc.depth);
    HIP_OR_RET(ctx, grow(d, d.rad_work, rt::radiance_work_bytes()));
    const rt::RadianceOptions q = radiance_options(ctx, env, spp, max_bounce, flags);
    HIP_OR_RET(ctx, order_after_last(d, s));
    HIP_OR_RET(ctx, rt::launch_lens_radiance(sc, ctx->traversal, cam, npix, first, count, (float4*)d_state,
                                             lens_options(lens), q, d.rad_work.p, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}

int lens_rays_check(rt_ctx* ctx, const float* cam, const rt_lens* lens, int64_t npix, int64_t first, int64_t count,
                    int sample0, int nsamples, const void* rays) {
    int st = camera_rays_check(ctx, cam, npix, first, count, rays);
    if (!st) st = lens_check(ctx, lens);
    if (st) return st;
    if (sample0 < 0) return set_err(ctx, RT_ERR_ARG, "sample0 %d < 0", sample0);
    if (nsamples < 1) return set_err(ctx, RT_ERR_ARG, "nsamples %d < 1", nsamples);
    if (count * (int64_t)nsamples >= ((int64_t)1 << 31))
        return set_err(ctx, RT_ERR_ARG, "%lld rays in one call: 2^31 or more", (long long)(count * (int64_t)nsamples));
    return RT_OK;
}

int lens_rays_enqueue(rt_ctx* ctx, Device& d, const float cam[10], const rt_lens* lens, int64_t npix, int64_t first,
                      int64_t count, int sample0, int nsamples, float* d_rays, hipStream_t s) {
    HIP_OR_RET(ctx, grow(d, d.rad_work, rt::radiance_work_bytes()));
    HIP_OR_RET(ctx, order_after_last(d, s));
    HIP_OR_RET(ctx, rt::launch_lens_rays(cam, npix, first, count, sample0, nsamples, lens_options(lens),
                                         (float4*)d_rays, d.rad_work.p, s));
    HIP_OR_RET(ctx, mark_launch(d, s));
    return RT_OK;
}
}  // namespace

int rt_lens_radiance_device(rt_ctx* ctx, int device_index, const float cam[10], const float env[5], const rt_lens* lens,
                            int64_t npix, int64_t first, int64_t count, int spp, int max_bounce, int flags,
                            rt_radiance_state* d_state, void* stream) {
    Device* dp = nullptr;
    int st = lens_radiance_check(ctx, cam, env, lens, npix, first, count, spp, max_bounce, flags, d_state);
    if (!st) st = slot_of(ctx, device_index, &dp);
    if (st) return st;
    if (count == 0) return RT_OK;
    if ((uintptr_t)d_state & 15) return set_err(ctx, RT_ERR_ARG, "d_state must be 16-byte aligned");
    HIP_OR_RET(ctx, hipSetDevice(dp->id));
    return lens_radiance_enqueue(ctx, *dp, cam, env, lens, npix, first, count, spp, max_bounce, flags, d_state,
                                 (hipStream_t)stream);
}

int rt_lens_radiance(rt_ctx* ctx, const float cam[10], const float env[5], const rt_lens* lens, int64_t npix,
                     int64_t first, int64_t count, int spp, int max_bounce, int flags, rt_radiance_state* state) {
    const int st = lens_radiance_check(ctx, cam, env, lens, npix, first, count, spp, max_bounce, flags, state);
    if (st) return st;
    if (count == 0) return RT_OK;
    // contiguous chunks over the slots; every slot is enqueued before any is waited for
    const int64_t nd = (int64_t)ctx->devs.size();
    for (int64_t k = 0; k < nd; ++k) {
        const int64_t b = count * k / nd, m = count * (k + 1) / nd - b;
        if (m <= 0) continue;
        Device& d = ctx->devs[k];
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, grow(d, d.rad_state, (size_t)m * sizeof(rt_radiance_state)));
        if (flags & RT_RADIANCE_RESUME)
            HIP_OR_RET(ctx, hipMemcpyAsync(d.rad_state.p, state + b, (size_t)m * sizeof(rt_radiance_state),
                                           hipMemcpyHostToDevice, d.stream));
        const int qs = lens_radiance_enqueue(ctx, d, cam, env, lens, npix, first + b, m, spp, max_bounce, flags,
                                             (rt_radiance_state*)d.rad_state.p, d.stream);
        if (qs) return qs;
        HIP_OR_RET(ctx, hipMemcpyAsync(state + b, d.rad_state.p, (size_t)m * sizeof(rt_radiance_state),
                                       hipMemcpyDeviceToHost, d.stream));
    }
    for (auto& d : ctx->devs) {
        HIP_OR_RET(ctx, hipSetDevice(d.id));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    }
    return RT_OK;
}

int rt_lens_rays_device(rt_ctx* ctx, int device_index, const float cam[10], const rt_lens* lens, int64_t npix,
                        int64_t first, int64_t count, int sample0, int nsamples, float* d_rays, void* stream) {
    Device* dp = nullptr;
    int st = lens_rays_check(ctx, cam, lens, npix, first, count, sample0, nsamples, d_rays);
    if (!st) st = slot_of(ctx, device_index, &dp);
    if (st) return st;
    if (count == 0) return RT_OK;
    if ((uintptr_t)d_rays & 15) return set_err(ctx, RT_ERR_ARG, "d_rays must be 16-byte aligned");
    HIP_OR_RET(ctx, hipSetDevice(dp->id));
    return lens_rays_enqueue(ctx, *dp, cam, lens, npix, first, count, sample0, nsamples, d_rays, (hipStream_t)stream);
}

int rt_lens_rays(rt_ctx* ctx, const float cam[10], const rt_lens* lens, int64_t npix, int64_t first, int64_t count,
                 int sample0, int nsamples, float* rays) {
    const int st = lens_rays_check(ctx, cam, lens, npix, first, count, sample0, nsamples, rays);
    if (st) return st;
    if (count == 0) return RT_OK;
    Device& d = ctx->devs[0];
    const size_t bytes = (size_t)count * (size_t)nsamples * 32;
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, grow(d, d.q_rays, bytes));
    const int qs = lens_rays_enqueue(ctx, d, cam, lens, npix, first, count, sample0, nsamples, (float*)d.q_rays.p,
                                     d.stream);
    if (qs) return qs;
    HIP_OR_RET(ctx, hipMemcpyAsync(rays, d.q_rays.p, bytes, hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

int rt_radiance_resolve_device(rt_ctx* ctx, int device_index, const rt_radiance_state* d_state, int64_t n,
                               float* d_rgb, void* stream) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (n < 0 || n >= ((int64_t)1 << 31)) return set_err(ctx, RT_ERR_ARG, "record count %lld out of range", (long long)n);
    if (n > 0 && (!d_state || !d_rgb)) return set_err(ctx, RT_ERR_ARG, "d_state / d_rgb must not be NULL");
    Device* dp = nullptr;
    const int st = slot_of(ctx, device_index, &dp);
    if (st) return st;
    if (n == 0) return RT_OK;
    const uintptr_t s0 = (uintptr_t)d_state, o0 = (uintptr_t)d_rgb;
    if ((s0 & 15) || (o0 & 3)) return set_err(ctx, RT_ERR_ARG, "d_state must be 16-byte and d_rgb 4-byte aligned");
    if (s0 < o0 + (uintptr_t)n * 12 && o0 < s0 + (uintptr_t)n * sizeof(rt_radiance_state))
        return set_err(ctx, RT_ERR_ARG, "d_state and d_rgb must not overlap");
    HIP_OR_RET(ctx, hipSetDevice(dp->id));
    const hipStream_t s = (hipStream_t)stream;
    HIP_OR_RET(ctx, order_after_last(*dp, s));
    HIP_OR_RET(ctx, rt::launch_resolve((const float4*)d_state, n, d_rgb, s));
    HIP_OR_RET(ctx, mark_launch(*dp, s));
    return RT_OK;
}

int rt_debug_accum_state(rt_ctx* ctx, rt_radiance_state* out) {
    const int open = accum_host_open(ctx, "rt_debug_accum_state");
    if (open) return open;
    if (!out) return set_err(ctx, RT_ERR_ARG, "rt_debug_accum_state: out must not be NULL");
    for (const auto& d : ctx->devs) {
        const int st = accum_slot_usable(ctx, d, "rt_debug_accum_state");
        if (st) return st;
    }
    return accum_gather_host(ctx, out, sizeof(rt_radiance_state), [](Device& d) { return (const void*)d.accum.p; });
}

int rt_debug_math(rt_ctx* ctx, int fn, const float* x, const float* y, float* out, int64_t n) {
    if (!ctx || !x || !out || n < 0) return set_err(ctx, RT_ERR_ARG, "bad arguments");
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    const size_t bytes = (size_t)n * sizeof(float);
    if (!bytes) return RT_OK;
    HIP_OR_RET(ctx, grow(d, d.scratch_a, 3 * bytes));
    float* dx = (float*)d.scratch_a.p;
    float* dy = dx + n;
    float* dout = dy + n;
    HIP_OR_RET(ctx, hipMemcpyAsync(dx, x, bytes, hipMemcpyHostToDevice, d.stream));
    if (y) HIP_OR_RET(ctx, hipMemcpyAsync(dy, y, bytes, hipMemcpyHostToDevice, d.stream));
    else HIP_OR_RET(ctx, hipMemsetAsync(dy, 0, bytes, d.stream));
    HIP_OR_RET(ctx, rt::launch_debug_math(fn, dx, dy, dout, n, d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

int rt_debug_fn(rt_ctx* ctx, int fn, const float* in, float* out, int64_t n) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    const int wi = rt::debug_fn_in(fn), wo = rt::debug_fn_out(fn);
    if (wi == 0) return set_err(ctx, RT_ERR_ARG, "no device function %d", fn);
    if (!in || !out || n < 0 || n > INT32_MAX) return set_err(ctx, RT_ERR_ARG, "bad arguments");
    if (fn == RT_FN_IBL && !ctx->have_env) return set_err(ctx, RT_ERR_STATE, "no environment");
    if (fn == RT_FN_CAMERA)   // camera_dir divides by the width (check_frame's condition on a frame's cam)
        for (int64_t i = 0; i < n; ++i)
            if (!(in[wi * i + 6] >= 1.0f && in[wi * i + 6] < 2147483648.0f))
                return set_err(ctx, RT_ERR_ARG, "item %lld: width %g", (long long)i, (double)in[wi * i + 6]);
    if (!n) return RT_OK;
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    const size_t ibytes = (size_t)n * wi * sizeof(float);
    const size_t obytes = ((size_t)n * wo * sizeof(float) + 15) & ~(size_t)15;
    HIP_OR_RET(ctx, grow(d, d.scratch_a, ibytes));
    HIP_OR_RET(ctx, grow(d, d.scratch_b, obytes + rt::debug_fn_scratch_bytes(fn, n)));
    HIP_OR_RET(ctx, hipMemcpyAsync(d.scratch_a.p, in, ibytes, hipMemcpyHostToDevice, d.stream));
    HIP_OR_RET(ctx, order_after_last(d, d.stream));
    HIP_OR_RET(ctx, rt::launch_debug_fn(dev_scene(ctx, d), fn, (const float*)d.scratch_a.p, (float*)d.scratch_b.p, n,
                                        (char*)d.scratch_b.p + obytes, d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(out, d.scratch_b.p, (size_t)n * wo * sizeof(float), hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

int rt_debug_trace(rt_ctx* ctx, int traversal, const float* rays, float* out, int64_t n) {
    if (!ctx || !rays || !out || n < 0) return set_err(ctx, RT_ERR_ARG, "bad arguments");
    if (!ctx->have_scene) return set_err(ctx, RT_ERR_STATE, "no scene");
    if (traversal == RT_TRAVERSAL_FAST && !ctx->hs.fast_ok)
        return set_err(ctx, RT_ERR_STATE, "FAST traversal unavailable for this scene");
    if (!n) return RT_OK;
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, grow(d, d.scratch_a, (size_t)n * 6 * sizeof(float)));
    HIP_OR_RET(ctx, grow(d, d.scratch_b, (size_t)n * 2 * sizeof(float)));
    HIP_OR_RET(ctx, hipMemcpyAsync(d.scratch_a.p, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, d.stream));
    HIP_OR_RET(ctx, order_after_last(d, d.stream));
    HIP_OR_RET(ctx, rt::launch_debug_trace(dev_scene(ctx, d), traversal, (const float*)d.scratch_a.p,
                                           (float*)d.scratch_b.p, n, d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(out, d.scratch_b.p, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

int rt_debug_trace_clustered(rt_ctx* ctx, const float* rays, float* out, int64_t n, int32_t info[4]) {
    if (!ctx || !rays || !out || !info || n < 0) return set_err(ctx, RT_ERR_ARG, "bad arguments");
    if (!ctx->have_scene) return set_err(ctx, RT_ERR_STATE, "no scene");
    // no fall-back to another trace: the hook runs the clustered loop or nothing
    if (ctx->hs.nbrute <= 0 || ctx->hs.ncluster <= 0)
        return set_err(ctx, RT_ERR_ARG, "the scene has no clustered brute-force array (%d records, %d clusters; option "
                       "\"brute_cluster\" %d)", (int)ctx->hs.nbrute, (int)ctx->hs.ncluster, ctx->brute_cluster);
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    HIP_OR_RET(ctx, grow(d, d.scratch_a, (size_t)n * 6 * sizeof(float)));
    HIP_OR_RET(ctx, grow(d, d.scratch_b, (size_t)n * 2 * sizeof(float)));
    if (n) HIP_OR_RET(ctx, hipMemcpyAsync(d.scratch_a.p, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, d.stream));
    HIP_OR_RET(ctx, order_after_last(d, d.stream));
    HIP_OR_RET(ctx, rt::launch_debug_trace_clustered(dev_scene(ctx, d), (const float*)d.scratch_a.p,
                                                     (float*)d.scratch_b.p, n, info, d.stream));
    if (n) HIP_OR_RET(ctx, hipMemcpyAsync(out, d.scratch_b.p, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

int rt_debug_pixel_log(rt_ctx* ctx, int traversal, const float cam[10], const float env[5], int64_t npix, int spp,
                       int max_bounce, int64_t pixel, float* log, int cap, int* n_events, float out3[3]) {
    rt::FrameParams fp;
    if (!cam) return set_err(ctx, RT_ERR_ARG, "null cam");
    const int W = (int)cam[6];
    if (W <= 0 || pixel < 0 || pixel >= npix) return set_err(ctx, RT_ERR_ARG, "pixel out of range");
    int st = check_frame(ctx, cam, env, npix, spp, 0, (int)(pixel / W), (int)npix, &fp);
    if (st) return st;
    if (!log || cap <= 0 || !n_events || !out3) return set_err(ctx, RT_ERR_ARG, "bad log buffer");
    if (traversal == RT_TRAVERSAL_FAST && !ctx->hs.fast_ok) traversal = RT_TRAVERSAL_REF;
    fp.max_bounce = max_bounce;   // (this entry point has never bounded it: check_frame got 0)
    fp.sun_skip = 0;   // the event log records every ray the reference traces, with its closest hit
    fp.sun_any = 0;
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    const size_t obytes = (size_t)fp.nloc * 3 * sizeof(float);
    const size_t lbytes = (size_t)cap * 16 * sizeof(float);
    HIP_OR_RET(ctx, grow(d, d.scratch_a, obytes + lbytes + 16));
    float* dout = (float*)d.scratch_a.p;
    fp.log_buf = dout + fp.nloc * 3;
    fp.log_count = (int32_t*)(fp.log_buf + (size_t)cap * 16);
    fp.log_cap = cap;
    fp.log_pixel = pixel;
    HIP_OR_RET(ctx, hipMemsetAsync(fp.log_count, 0, sizeof(int32_t), d.stream));
    HIP_OR_RET(ctx, order_after_last(d, d.stream));
    HIP_OR_RET(ctx, rt::launch_debug_log(dev_scene(ctx, d), fp, traversal, dout, (unsigned int*)d.work.p, d.stream));
    HIP_OR_RET(ctx, mark_launch(d, d.stream));
    int32_t n = 0;
    HIP_OR_RET(ctx, hipMemcpyAsync(&n, fp.log_count, sizeof n, hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    if (n > cap) n = cap;
    HIP_OR_RET(ctx, hipMemcpy(log, fp.log_buf, (size_t)n * 16 * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OR_RET(ctx, hipMemcpy(out3, dout + 3 * (pixel % W), 3 * sizeof(float), hipMemcpyDeviceToHost));
    *n_events = n;
    return RT_OK;
}

int rt_debug_brute_slices(int64_t nloc, int64_t lanes, int spp, int option, int accum_base, int32_t out[3]) {
    if (!out || nloc < 0 || lanes < 0 || option < -1 || option > 16) return RT_ERR_ARG;
    const int todo = spp - std::max(accum_base, 0);
    const int v = rt::brute_slice_launch(rt::brute_slice_offer(option, todo, accum_base >= 0), nloc, lanes);
    out[0] = v != 0;
    out[1] = v & 0xff;
    out[2] = v >> 8;
    return RT_OK;
}

int rt_debug_last_slices(void) { return rt::last_launch().slices; }

int rt_debug_last_direct(void) { return rt::last_launch().direct; }

int rt_debug_shell_word(rt_ctx* ctx) {
    if (!ctx || !ctx->have_scene || ctx->hs.nshell <= 0 || ctx->hs.brute_shell.size() < 8) return 0;
    int32_t w;
    std::memcpy(&w, &ctx->hs.brute_shell[7], sizeof w);
    return w;
}

int rt_debug_last_launch(int32_t out[21]) {
    if (!out) return RT_ERR_ARG;
    const rt::LaunchNote n = rt::last_launch();
    const rt::KernelKey& k = n.key;
    const int64_t v[21] = {k.trav, k.count, k.log,  k.smem,       k.ovf,    k.resume, k.step, k.wide,          k.brute,
                           k.ts,   k.acc,   n.team, n.walk_team,  n.slices, n.refill, n.grid, (int64_t)n.lds,
                           n.shell, n.near, n.quad, n.primary};
    for (int i = 0; i < 21; ++i) out[i] = (int32_t)std::min<int64_t>(v[i], INT32_MAX);
    return RT_OK;
}

static_assert(RT_SPEC_PICK == rt::kSpecPick, "rt_debug.h states the pick word's trail code");

int rt_debug_pilot_order(rt_ctx* ctx, const uint32_t* cost, int64_t n, int chunk, int levels, int pilot, int max_bounce,
                         uint32_t* order_out) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (!cost || !order_out) return set_err(ctx, RT_ERR_ARG, "rt_debug_pilot_order: cost and order_out must not be NULL");
    // (the ranges of the options "pilot_chunk", "pilot_levels" and "pilot" and of a frame's maxBounce)
    if (n <= 0 || n > INT32_MAX || chunk < 1 || chunk > 4096 || levels < 2 || levels > 256 || pilot < 1 ||
        pilot > (1 << 20) || max_bounce > 4096)
        return set_err(ctx, RT_ERR_ARG, "rt_debug_pilot_order: n %lld, chunk %d, levels %d, pilot %d, maxBounce %d",
                       (long long)n, chunk, levels, pilot, max_bounce);
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    // scratch_a: a two-pass launch's scratch for a tile of n pixels, the cost and the order where it has them
    const rt::PilotLayout L = rt::pilot_layout((size_t)n);
    HIP_OR_RET(ctx, grow(d, d.scratch_a, L.need));
    uint32_t* dcost = (uint32_t*)((char*)d.scratch_a.p + L.cost);
    uint32_t* dorder = (uint32_t*)((char*)d.scratch_a.p + L.order);
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    HIP_OR_RET(ctx, hipMemcpyAsync(dcost, cost, bytes, hipMemcpyHostToDevice, d.stream));
    HIP_OR_RET(ctx, rt::launch_pilot_order(dcost, n, chunk, levels, pilot, max_bounce, dorder, d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(order_out, dorder, bytes, hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

int rt_debug_pilot_pick(rt_ctx* ctx, const uint32_t* cost, int64_t n, int64_t lanes, int spec, int32_t out[2]) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (!cost || !out || n <= 0 || n > INT32_MAX || lanes < 1 || lanes > ((int64_t)1 << 40) || spec < 0 || spec > 1)
        return set_err(ctx, RT_ERR_ARG, "rt_debug_pilot_pick: n %lld, lanes %lld, spec %d", (long long)n,
                       (long long)lanes, spec);
    Device& d = ctx->devs[0];
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    HIP_OR_RET(ctx, grow(d, d.scratch_a, bytes));
    HIP_OR_RET(ctx, grow(d, d.scratch_b, 2 * sizeof(int32_t)));
    unsigned* left = (unsigned*)d.scratch_b.p;
    HIP_OR_RET(ctx, hipMemcpyAsync(d.scratch_a.p, cost, bytes, hipMemcpyHostToDevice, d.stream));
    HIP_OR_RET(ctx, rt::launch_pilot_pick((const uint32_t*)d.scratch_a.p, n, lanes, spec, left, (int*)(left + 1), d.stream));
    HIP_OR_RET(ctx, hipMemcpyAsync(out, left, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
    HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

int rt_debug_last_pilot(rt_ctx* ctx, int64_t info[8], uint32_t* cost_out, uint32_t* order_out, int64_t cap) {
    if (!ctx) return set_err(nullptr, RT_ERR_ARG, "null context");
    if (!info || cap < 0 || (cap > 0 && (!cost_out || !order_out)))
        return set_err(ctx, RT_ERR_ARG, "rt_debug_last_pilot: bad arguments");
    if (ctx->devs.size() != 1) return set_err(ctx, RT_ERR_ARG, "rt_debug_last_pilot: a single-device context only");
    Device& d = ctx->devs[0];
    const rt::PilotNote& note = d.pilot_note;
    if (!note.two_pass || !d.pilot.p || !d.work.p)
        return set_err(ctx, RT_ERR_STATE, "rt_debug_last_pilot: the last render launch ran one pass");
    HIP_OR_RET(ctx, hipSetDevice(d.id));
    if (d.pending) HIP_OR_RET(ctx, hipEventSynchronize(d.done));
    const rt::PilotLayout L = rt::pilot_layout((size_t)note.nloc);
    const uint32_t* dcost = (const uint32_t*)((const char*)d.pilot.p + L.cost);
    int32_t lp[2] = {0, 0};   // pixels left, pick word
    if (note.lanes > 0) {
        HIP_OR_RET(ctx, hipMemcpy(lp, (const char*)d.work.p + rt::kTeamOffset, sizeof lp, hipMemcpyDeviceToHost));
    } else {
        // no pick ran: the count kernel over the costs here, on words of this hook's own (the pick word stays 0)
        HIP_OR_RET(ctx, grow(d, d.scratch_b, sizeof lp));
        unsigned* left = (unsigned*)d.scratch_b.p;
        HIP_OR_RET(ctx, rt::launch_pilot_pick(dcost, note.nloc, 1, 0, left, (int*)(left + 1), d.stream));
        HIP_OR_RET(ctx, hipMemcpyAsync(lp, left, sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
        HIP_OR_RET(ctx, hipStreamSynchronize(d.stream));
    }
    const int64_t v[8] = {1, note.nloc, note.pilot, note.chunk, note.levels, note.lanes, (uint32_t)lp[0], lp[1]};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    const size_t bytes = (size_t)std::min<int64_t>(cap, note.nloc) * sizeof(uint32_t);
    if (bytes) {
        HIP_OR_RET(ctx, hipMemcpy(cost_out, dcost, bytes, hipMemcpyDeviceToHost));
        HIP_OR_RET(ctx, hipMemcpy(order_out, (const char*)d.pilot.p + L.order, bytes, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

int rt_debug_brute_refill(int64_t nloc, int64_t lanes, int option, int32_t* out) {
    if (!out || nloc < 0 || lanes < 0 || option < -1 || option > rt::kRefillMax) return RT_ERR_ARG;
    *out = rt::brute_refill_launch(option, nloc, lanes);
    return RT_OK;
}

int rt_debug_brute_lean(const float* mat, int64_t nmat6, const float env[5], const int32_t frame[7],
                        const int32_t kernel[6], int32_t out[2]) {
    if ((nmat6 > 0 && !mat) || nmat6 < 0 || nmat6 % 6 || !env || !frame || !kernel || !out) return RT_ERR_ARG;
    if (frame[6] < -1 || frame[6] > 1) return RT_ERR_ARG;
    out[0] = rt::materials_diffuse_only(mat, nmat6) ? 1 : 0;
    rt::FrameParams fp{};
    std::memcpy(fp.env, env, sizeof fp.env);
    fp.spp = frame[0];
    fp.max_bounce = frame[1];
    fp.pass = frame[2];
    fp.pilot = frame[3];
    fp.fixed_point = frame[4];
    fp.sun_cache = frame[4] && frame[5] ? 1 : 0;   // (as check_frame makes it)
    rt::KernelKey k{kernel[5], kernel[2], kernel[3], 0, 0, 0, 1, 0, kernel[0], 1, kernel[4]};
    out[1] = rt::brute_lean_kernel(k, kernel[1]) && rt::brute_lean_frame(out[0] && frame[6] != 0 ? rt::kHostLean : 0, fp);
    return RT_OK;
}

int rt_debug_last_refill(int64_t out[3]) {
    if (!out) return RT_ERR_ARG;
    out[0] = rt::last_launch().refill;
    out[1] = g_refill_events.load(std::memory_order_relaxed);
    out[2] = g_refill_lanes.load(std::memory_order_relaxed);
    return RT_OK;
}

int rt_debug_timings(rt_ctx* ctx, double out[4]) {
    if (!ctx || !out) return set_err(ctx, RT_ERR_ARG, "bad arguments");
    out[0] = ctx->t_pack_ms;
    out[1] = ctx->t_upload_ms;
    out[2] = ctx->t_env_ms;
    out[3] = ctx->t_render_ms;
    return RT_OK;
}

int rt_debug_scene_info(rt_ctx* ctx, int64_t out[8]) {
    if (!ctx || !out) return set_err(ctx, RT_ERR_ARG, "bad arguments");
    out[0] = ctx->hs.fast_ok ? 1 : 0;
    out[1] = ctx->hs.depth;
    out[2] = ctx->hs.nnodes;
    out[3] = ctx->hs.ntri;
    out[4] = effective_traversal(ctx) == RT_TRAVERSAL_FAST ? ctx->hs.nbrute : 0;
    out[5] = out[4] ? ctx->hs.nbox : 0;
    // the 4-wide layout's origin bound of the origin-folded dequantisation, in millionths (0: none)
    out[6] = ctx->hs.wnodes.empty() ? 0 : (int64_t)std::llround((double)ctx->hs.wdq_omax * 1e6);
    out[7] = 0;
    return RT_OK;
}

}  // extern "C"
