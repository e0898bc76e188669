// Ray queries (rt_trace / rt_trace_device, include/rt_api.h): closest-hit and any-hit batches of the caller's
// own rays through the uploaded scene, on the walks the render kernels are made of (rt_device.h).  A
// translation unit of its own: the instantiations below join no other module, so the code objects of the
// render, accumulation, adaptive, denoise, speculation and debug kernels are what they were without it.
//
// A ray is two float4 (dir.xyz origin.x | origin.yz tmax reserved), a result one (k, tri bits, u, v).
// Every engine returns the hit of the frame's rayTrace under the same traversal, restricted to k < lim =
// fminf(tmax, 1000): the restriction is a filter on the unrestricted closest hit, so an engine may start its
// cull distance at lim (the tree walks: FastRay::bk) or compare at the end (brute force, REF, the plain form).
#include "rt_device.h"

namespace rt {

namespace {

struct QRay {
    rtm_f3 o, d;
    float lim;
};

__device__ __forceinline__ QRay load_ray(const float4* __restrict__ rays, unsigned i) {
    const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
    QRay r;
    r.d = rtm_v3(a.x, a.y, a.z);
    r.o = rtm_v3(a.w, b.x, b.y);
    r.lim = fminf(b.z, 1000.0f);   // a NaN tmax is dropped: the reference's horizon
    return r;
}

// The result of a walk that ended with (k, tri): a miss unless tri >= 0 and k < lim; on a hit the barycentrics
// of the winning triangle, recomputed from its tri_geo record in mt_test's operation order with the IEEE
// 1.0f / a -- once per ray, whichever engine found the triangle.
__device__ __forceinline__ float4 make_result(const DevScene& S, const QRay& r, float k, int tri) {
    if (tri < 0 || !(k < r.lim)) return make_float4(1000.0f, __int_as_float(-1), 0.0f, 0.0f);
    const float4 g0 = S.tri_geo[3 * tri + 0];
    const float4 g1 = S.tri_geo[3 * tri + 1];
    const float4 g2 = S.tri_geo[3 * tri + 2];
    const rtm_f3 e1 = xyz(g1), e2 = xyz(g2);
    const rtm_f3 h = rtm_cross(r.d, e2);
    const float a = rtm_dot(e1, h);
    const float f = 1.0f / a;
    const rtm_f3 s = rtm_sub(r.o, xyz(g0));
    const float u = f * rtm_dot(s, h);
    const rtm_f3 q = rtm_cross(s, e1);
    const float v = f * rtm_dot(r.d, q);
    return make_float4(k, __int_as_float(tri), u, v);
}

// ---- the plain form: one thread per ray, trace<>, a grid over the rays, the whole stack in LDS ----
// (what debug_trace_kernel does, instantiated here; REF always runs this form: trace_ref has no early exit
// and is no hot path.  An any-hit query gets the closest hit, which is a hit with k < lim.)
template <int TRAV>
__global__ void __launch_bounds__(256) query_plain_kernel(DevScene S, const float4* __restrict__ rays,
                                                          float4* __restrict__ out, unsigned n) {
    extern __shared__ int lds_stack[];
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    Cnt c{};
    const QRay r = load_ray(rays, t);
    const Hit h = trace<TRAV, false>(S, S.nodes, S.tri_fast, r.o, r.d, lds_stack + threadIdx.x, blockDim.x,
                                     lane_stack(S, lds_stack), c);
    out[t] = make_result(S, r, h.k, h.tri);
}

// ---- the persistent tree walks: a lane keeps its FastRay across rounds (render_resume_kernel's pattern) ----
// The wave steps until resume_min / 64 of its lanes are free; the free lanes then store their result and take
// new rays: one atomic per wave reserves a contiguous run of `chunk` rays, which its refills hand out in order, so
// the two float4 loads per lane and the 16-byte stores coalesce.  No lane waits on another wave, so any grid size
// terminates.  The grid stays within kMaxLanesPerCu lanes per CU, so the scene's stack_ovf buffer covers it.
// WIDE: the 4-wide layout with the exact dequantisation only -- the origin-folded form (wide_step's DQ) is
// conservative only for origins within DevScene::wdq_omax, which a render checks once per camera and a query
// would have to check per ray.
template <bool OVF, bool WIDE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WIDE ? kWideWaves : 4)))
query_walk_kernel(DevScene S, const float4* __restrict__ rays, float4* __restrict__ out, unsigned n, int any,
                  int resume_min, unsigned chunk, unsigned* __restrict__ counter) {
    extern __shared__ int lds_stack[];
    Cnt c{};
    const LaneStack lst = lane_stack(S, lds_stack);
    const char* const nb = reinterpret_cast<const char*>(WIDE ? S.wnodes : S.nodes);
    const char* const tb = reinterpret_cast<const char*>(WIDE ? S.wleaves : S.tri_fast);
    const int lane = threadIdx.x & 63;
    FastRay T;
    T.item = 0; T.soff = 0; T.bk = 1000.0f; T.bt = -1; T.brank = -1; T.any = any != 0;
    T.o = rtm_v3(0, 0, 0); T.d = rtm_v3(0, 0, 1); T.ix = T.iy = T.iz = 0.0f;
    QRay r{};
    unsigned idx = 0;
    bool have = false, tracing = false, dry = false;   // dry is wave-uniform
    unsigned wnext = 0, wend = 0;                      // the wave's run of rays not yet handed to a lane (wave-uniform)
    while (true) {
        if (have && !tracing) {
            out[idx] = make_result(S, r, T.bk, WIDE ? (T.bt >= 0 ? (int)((unsigned)T.bt / 48u) : -1) : T.bt);
            have = false;
        }
        const unsigned long long need = __ballot(!tracing);
        if (!dry && need) {
            // the cnt free lanes take the rest of the wave's run and, when that is too short, the head of a new
            // run of `chunk` (>= 64) rays: one atomic per run, not per refill -- on one counter the atomics of
            // every wave serialise, and a refill hands out only about resume_min rays
            const unsigned cnt = (unsigned)__popcll(need), left = wend - wnext;
            const unsigned j = lane_prefix(need, 0u);
            unsigned my = wnext + j;
            bool valid = true;
            if (left < cnt) {
                const int first = __ffsll((long long)need) - 1;
                unsigned base = 0;
                if (lane == first) base = atomicAdd(counter, chunk);
                base = (unsigned)__shfl((int)base, first, 64);
                const unsigned rb = min(base, n), re = min(base + chunk, n);   // the new run, cut at the stream's end
                if (j >= left) my = rb + (j - left);
                valid = j < left || my < re;
                wnext = min(rb + (cnt - left), re);
                wend = re;
                dry = rb >= n;
            } else {
                wnext += cnt;
            }
            if (!tracing && valid) {
                idx = my;
                r = load_ray(rays, idx);
                have = true;
                tracing = !fast_init<false>(S, T, r.o, r.d, c) && r.lim > 0.0f;
                T.bk = r.lim;   // only a triangle with k < lim is accepted (an any-hit ray ends at the first)
                if (WIDE) T.item = S.wroot_ref;
            }
        }
        const unsigned long long alive = __ballot(have);
        if (alive == 0) {
            if (dry) break;
            continue;
        }
        if (__ballot(tracing) == 0) continue;
        const int rthr = resume_min * __popcll(alive);
        ItemData D;
        if (!WIDE && tracing) D = item_fetch<false>(T.item, nb, tb, 16u);
        while (true) {
            if (tracing && (WIDE ? wide_step<false, OVF, false>(T, nb, tb, lst, c)
                                 : fast_step_pipe<false, false, OVF>(T, D, nb, tb, lst, 16u, c)))
                tracing = false;
            const unsigned long long tr = __ballot(tracing);
            if (tr == 0 || 64 * __popcll(alive & ~tr) >= rthr) break;
        }
    }
}

// ---- brute force, a wave at a time: 64 rays, one lock-step trace over brute_box, 64 stores ----
// (the records read from global memory; no early exit: an any-hit query gets the closest hit)
__global__ void __launch_bounds__(256) query_brute_kernel(DevScene S, const float4* __restrict__ rays,
                                                          float4* __restrict__ out, unsigned n, unsigned chunk,
                                                          unsigned* __restrict__ counter) {
    extern __shared__ int lds_stack[];
    char* const wl = reinterpret_cast<char*>(lds_stack) + (threadIdx.x >> 6) * BRUTE_WAVE_LDS;
    const int lane = threadIdx.x & 63;
    Cnt c{};
    while (true) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(counter, chunk);   // a run of `chunk` rays (a multiple of 64) per atomic
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        if (base >= n) break;
        const unsigned end = min(base + chunk, n);
        for (unsigned b = base; b < end; b += 64u) {
            const unsigned i = b + lane;
            if (i < end) {
                const QRay r = load_ray(rays, i);
                const Hit h = trace_brute_compact<false, false>(S, r.o, r.d, wl, S.brute + 1, 4u, c);
                out[i] = make_result(S, r, h.k, h.tri);
            }
            wave_lds_sync();   // the next trace rewrites the wave's tables
        }
    }
}

}  // namespace

// the persistent form is the automatic choice of an engine only where it measured faster than the plain form
// on the same rays: its median below the plain form's by more than the plain form's max - min, on the frame's camera
// rays in pixel order and shuffled (tools/query_bench.py, profiles/r16_ray_query.json).  ms, plain /
// persistent, pixel order and shuffled:
//   4-wide walk, C5, 8.3 M rays:  2.45 / 1.27 and 4.39 / 1.64  -> persistent (any-hit rays of 5 % of the diagonal:
//                                 7.14 / 1.49: the plain form has no early exit)
//   BVH2 walk, C3, 1 M rays:      0.139 / 0.323 and 0.201 / 0.326  -> plain
//   brute force, C2, 1 M rays:    0.031 / 0.293 and 0.035 / 0.293  -> plain
// (1 M rays are 4 per resident lane, and a run is then 64 rays: both persistent forms take about 0.3 ms whatever
// the engine walks -- presumably the 16 K atomics on one counter; not profiled)
constexpr bool kQueryAutoPersistentBvh2 = false, kQueryAutoPersistentWide = true, kQueryAutoPersistentBrute = false;

hipError_t launch_query(const DevScene& sc, int traversal, int any, const float4* rays, float4* out, int64_t n,
                        const QueryOptions& q, unsigned int* counter, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    int block = q.block;
    const bool fast = traversal == TRAV_FAST && sc.ntri > 0;
    const bool brute = fast && sc.nbrute > 0;
    // the 4-wide walk where choose_kernel takes it: the layout is in use and the scene is not one a render stages
    const size_t scene_bytes = (size_t)(kNodeF4 * sc.nnodes + 3 * sc.ntri) * sizeof(float4);
    const bool wide = fast && !brute && sc.wnodes && !(scene_bytes <= kLdsSceneMax && sc.stack_lds >= sc.depth);
    const bool persistent = fast && (q.engine == 2 || (q.engine == 0 && (brute ? kQueryAutoPersistentBrute
                                                                          : wide ? kQueryAutoPersistentWide
                                                                                 : kQueryAutoPersistentBvh2)));
    if (!persistent) {
        // not a persistent grid: the whole FAST stack lives in LDS (no overflow buffer sized for this grid)
        DevScene s2 = sc;
        s2.stack_lds = sc.depth > 0 ? sc.depth : 1;
        s2.stack_ovf = nullptr;
        const int trav = traversal == TRAV_REF ? TRAV_REF : TRAV_FAST;
        while (block > 64 && stack_lds_bytes(s2, trav, block) > 64 * 1024) block /= 2;
        const size_t lds = stack_lds_bytes(s2, trav, block);
        int64_t grid = (n + block - 1) / block;
        const dim3 g((unsigned)grid), b((unsigned)block);
        const unsigned un = (unsigned)n;
        if (trav == TRAV_REF) hipLaunchKernelGGL(query_plain_kernel<TRAV_REF>, g, b, lds, stream, s2, rays, out, un);
        else hipLaunchKernelGGL(query_plain_kernel<TRAV_FAST>, g, b, lds, stream, s2, rays, out, un);
        return hipGetLastError();
    }
    const bool ovf = !brute && sc.stack_lds < sc.depth;
    const void* fn = brute ? (const void*)query_brute_kernel
                     : wide ? (ovf ? (const void*)query_walk_kernel<true, true> : (const void*)query_walk_kernel<false, true>)
                            : (ovf ? (const void*)query_walk_kernel<true, false> : (const void*)query_walk_kernel<false, false>);
    const size_t lds = stack_lds_bytes(sc, TRAV_FAST, block);
    hipError_t e = hipSuccess;
    const int64_t resident = resident_blocks(fn, block, lds, q.max_waves, &e);
    if (e != hipSuccess) return e;
    int64_t grid = std::min<int64_t>((n + block - 1) / block, resident);
    if (q.grid_cap > 0) grid = std::min<int64_t>(grid, q.grid_cap);
    e = hipMemsetAsync(counter, 0, sizeof(unsigned int), stream);
    if (e != hipSuccess) return e;
    // rays a wave reserves per atomic: a quarter of its share of the stream, in whole waves of 64, at most 512 (all
    // waves add to one counter: with 64 per atomic C3's 1 M rays spent 0.3 ms in them alone; a long run also keeps
    // a wave on neighbouring rays, a short one keeps the stream's tail spread over the grid)
    const int64_t waves = grid * (block / 64);
    unsigned chunk = (unsigned)std::min<int64_t>(512, std::max<int64_t>(64, n / waves / 4 / 64 * 64));
    DevScene a0 = sc;
    unsigned un = (unsigned)n;
    int a_any = any, a_rmin = q.resume_min;
    void* wargs[] = {&a0, &rays, &out, &un, &a_any, &a_rmin, &chunk, &counter};
    void* bargs[] = {&a0, &rays, &out, &un, &chunk, &counter};
    return hipLaunchKernel(fn, dim3((unsigned)grid), dim3((unsigned)block), brute ? bargs : wargs, lds, stream);
}

}  // namespace rt
