// Radiance queries (rt_radiance / rt_radiance_device, rt_camera_rays*, include/rt_api.h): the integrator of a frame
// (naiveGI, Raytracing.cl:46-151, under the sample loop of Raytracing.cl:184-209) run on the caller's own rays with
// the caller's own RNG seeds.  A translation unit of its own, like rt_query.hip: the instantiations below join no
// other module, so the code objects of every other kernel are what they were without it.
//
// A ray is two float4 (dir.xyz origin.x | origin.yz seed0 seed1: rt_trace's first six words, the seeds' bits where
// rt_trace has tmax and reserved), a result the accumulation's 32-byte state record (save_state, rt_kernels.hip):
// sum.xyz k | seed0 seed1 tri n.  The contract: the query of a frame's camera rays with that frame's seeds is that
// frame, bit for bit -- the loop below is render_kernel's, with the first ray and the seeds read from memory.
#include "rt_device.h"

namespace rt {

namespace {

// bits of radiance_kernel's `flags`
constexpr int kRadResume = 1;      // RT_RADIANCE_RESUME: the record is read, no first ray is traced
constexpr int kRadSunSkip = 2;     // FrameParams::sun_skip, as check_frame makes it
constexpr int kRadFixedPoint = 4;  // FrameParams::fixed_point
constexpr int kRadSunCache = 8;    // FrameParams::sun_cache

// Persistent wave64, render_kernel's state machine (PRIMARY / PREP / BOUNCE / SUN; FETCH: the lane holds no ray):
// every round each busy lane traces one ray.  A lane that finishes its ray stores the record and takes the next ray
// of its wave's run -- query_walk_kernel's hand-out: one atomic reserves `chunk` consecutive rays for the wave, its
// refills hand them out in order, so the two float4 loads per ray and the record stores of a refill coalesce.  No
// lane waits on another wave: any grid size terminates.
// The traversal is trace<>: REF's DFS; on a brute-force scene the global records with the wave's LDS area
// (query_brute_kernel's form); else trace_fast over the BVH2 nodes with the whole stack in LDS (launch_radiance).
// Shortcuts carried over from the render loop, FAST only as there, none of which changes a bit: an unlit sun's
// shadow ray is not traced (kRadSunSkip), a sample that drew no random number is summed for the rest of the call
// (kRadFixedPoint), the first bounce's shadow ray is traced once per call (kRadSunCache; a resumed record does not
// carry it, so each call traces it once).
template <int TRAV>
__global__ void __launch_bounds__(256) radiance_kernel(DevScene S, const float4* __restrict__ rays,
                                                       float4* __restrict__ state, unsigned n, int spp, int maxB,
                                                       float e3, float e4, int flags, unsigned chunk,
                                                       unsigned* __restrict__ counter,
                                                       const LaunchConst* __restrict__ lconst) {
    extern __shared__ __attribute__((aligned(16))) int lds_stack[];
    const int B = blockDim.x;
    int* stk = lds_stack + threadIdx.x;
    const LaneStack lst = lane_stack(S, lds_stack);
    Cnt c{};
    const LaunchConst& C = *lconst;   // uniform: the sun vector and the IBL's rotations
    const int lane = threadIdx.x & 63;
    const bool resume = (flags & kRadResume) != 0;
    const bool sun_skip = TRAV == TRAV_FAST && (flags & kRadSunSkip) != 0;
    const bool fixed_point = TRAV == TRAV_FAST && (flags & kRadFixedPoint) != 0;
    const bool sun_cache = TRAV == TRAV_FAST && (flags & kRadSunCache) != 0;

    int phase = FETCH;
    unsigned idx = 0;
    uint32_t seed0 = 0, seed1 = 0;
    rtm_f3 co = rtm_v3(0, 0, 0), cd = rtm_v3(0, 0, 1);   // the caller's ray
    float kc = 1000.0f;                                  // its hit
    int tc = -1;
    rtm_f3 so = rtm_v3(1, 1, 1);
    float k = 1000.0f;
    int tri = -1, j = 0;
    rtm_f3 Bo = rtm_v3(0, 0, 0), Bd = rtm_v3(0, 0, 0);
    rtm_f3 acc = rtm_v3(0, 0, 0);
    int s = 0, slim = 0;
    int sun0 = -2;   // the first bounce's shadow-ray hit (-1 = miss; -2 = not traced yet)
    bool dry = false;                  // wave-uniform: the stream is handed out
    unsigned wnext = 0, wend = 0;      // the wave's run of rays not yet handed to a lane (wave-uniform)

    auto finish_ray = [&]() __attribute__((always_inline)) {
        state[2 * (size_t)idx] = make_float4(acc.x, acc.y, acc.z, kc);
        state[2 * (size_t)idx + 1] =
            make_float4(__uint_as_float(seed0), __uint_as_float(seed1), __int_as_float(tc), __int_as_float(s));
        phase = FETCH;
    };

    while (true) {
        if (TRAV == TRAV_FAST && S.nbrute > 0) wave_lds_sync();   // (brute force: the next trace rewrites the wave's tables)
        const unsigned long long need = __ballot(phase == FETCH);
        if (!dry && need) {
            // query_walk_kernel's hand-out: the free lanes take the rest of the wave's run and, when that is too
            // short, the head of a new run of `chunk` (>= 64) rays
            const unsigned cnt = (unsigned)__popcll(need), left = wend - wnext;
            const unsigned r = lane_prefix(need, 0u);
            unsigned my = wnext + r;
            bool valid = true;
            if (left < cnt) {
                const int first = __ffsll((long long)need) - 1;
                unsigned base = 0;
                if (lane == first) base = atomicAdd(counter, chunk);
                base = (unsigned)__shfl((int)base, first, 64);
                const unsigned rb = min(base, n), re = min(base + chunk, n);   // the new run, cut at the stream's end
                if (r >= left) my = rb + (r - left);
                valid = r < left || my < re;
                wnext = min(rb + (cnt - left), re);
                wend = re;
                dry = rb >= n;
            } else {
                wnext += cnt;
            }
            if (phase == FETCH && valid) {
                idx = my;
                const float4 a = rays[2 * (size_t)idx], b = rays[2 * (size_t)idx + 1];
                cd = rtm_v3(a.x, a.y, a.z);
                co = rtm_v3(a.w, b.x, b.y);
                sun0 = -2;
                if (resume) {
                    // the record in place of a first ray; no index comes from it unchecked: a tri outside [0, T) is a miss
                    const float4 u = state[2 * (size_t)idx], v = state[2 * (size_t)idx + 1];
                    acc = rtm_v3(u.x, u.y, u.z);
                    kc = u.w;
                    seed0 = __float_as_uint(v.x);
                    seed1 = __float_as_uint(v.y);
                    tc = __float_as_int(v.z);
                    if ((unsigned)tc >= (unsigned)S.ntri) tc = -1;
                    s = __float_as_int(v.w);
                    tri = tc; j = 0;
                    so = rtm_v3(1, 1, 1);
                    phase = PREP;
                } else {
                    acc = rtm_v3(0, 0, 0);
                    seed0 = __float_as_uint(b.z);
                    seed1 = __float_as_uint(b.w);
                    s = 0;
                    phase = PRIMARY;
                }
                slim = (int)((unsigned)s + (unsigned)spp);
            }
        }
        if (__ballot(phase != FETCH) == 0) {
            if (dry) break;
            continue;
        }
        if (phase == FETCH) continue;

        if (phase == PREP) {
            // naiveGI loop head for bounce j (Raytracing.cl:46-79); may complete samples without tracing
            bool done = true;
            const bool cam = j == 0;
            const rtm_f3 Ro = cam ? co : Bo, Rd = cam ? cd : Bd;
            const float kh = cam ? kc : k;
            if (j > maxB) {
                // naiveGI's loop never entered (maxBounce < 0): the sample stays 1
            } else if (tri < 0) {
                so = rtm_scale(rtm_mul(so, sample_ibl_if<false>(S, C, Rd, e4, c)), e4);
            } else {
                const float4 sh = S.tri_shade[tri];
                const rtm_f3 nrm = xyz(sh);
                const Mat cm = load_mat(S.mat, __float_as_int(sh.w));
                if (cm.type == 0) {
                    so = rtm_scale(so, cm.rough);
                } else {
                    const float4 f2 = S.tri_frame[3 * tri + 2];
                    const rtm_f3 nn = xyz(f2);
                    float invPdf = 0.0f;
                    rtm_f3 brdf = rtm_v3(0, 0, 0);
                    if (cm.type == 1) {
                        Bd = hemi_cosine(nrm, S.tri_frame[3 * tri], S.tri_frame[3 * tri + 1], f2, &seed1, &seed0, &invPdf);
                        brdf = rtm_scale(cm.color, 1.0f / 3.14f);
                    } else if (cm.type == 2) {
                        Bd = hemi_uniform(nrm, S.tri_frame[3 * tri], S.tri_frame[3 * tri + 1], f2, &seed1, &seed0, &invPdf);
                        brdf = brdf_ggx(cm.color, cm.rough, rtm_scale(Rd, -1.0f), Bd, nrm);
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
                acc = rtm_add(acc, so);
                ++s;
                // a sample that ends at its first loop head drew no random number: every later sample of the call
                // is this sample again, added in order (FrameParams::fixed_point)
                if (fixed_point && j == 0)
                    for (; s < slim; ++s) acc = rtm_add(acc, so);
                if (s >= slim) {
                    finish_ray();
                } else {
                    tri = tc; j = 0;
                    so = rtm_v3(1, 1, 1);
                }
                continue;
            }
        }

        // -- one ray per busy lane --
        const rtm_f3 to = (phase == PRIMARY) ? co : Bo;
        const rtm_f3 td = (phase == PRIMARY) ? cd : ((phase == BOUNCE) ? Bd : C.sun);
        const Hit h = trace<TRAV, false>(S, S.nodes, S.tri_fast, to, td, stk, B, lst, c);
        bool finish = false;
        if (phase == PRIMARY) {
            // the first hit as rt_trace reports it: the row of faceData or -1, the distance or the horizon
            tc = h.tri >= 0 ? h.tri : -1;
            kc = h.tri >= 0 ? h.k : 1000.0f;
            tri = tc; j = 0;
            so = rtm_v3(1, 1, 1);
            phase = PREP;
            continue;
        }
        int sun_hit = -2;   // the shadow ray's hit for the sun term below (-1 = miss; -2 = no sun term now)
        const bool sun_first = sun_cache && j == 0;
        if (phase == BOUNCE) {
            if (h.tri >= 0) {
                tri = h.tri; k = h.k;
                const Mat bm = load_mat(S.mat, __float_as_int(S.tri_shade[h.tri].w));
                if (bm.type != 0) {
                    if (j == maxB) {
                        so = rtm_v3(0, 0, 0);
                        finish = true;
                    } else {
                        ++j;
                        phase = PREP;
                    }
                } else {
                    so = rtm_scale(so, bm.rough);
                    finish = true;
                }
            } else if (sun_skip) {
                sun_hit = -1;   // unlit sun: the shadow ray cannot change the sample
            } else if (sun_first && sun0 != -2) {
                sun_hit = sun0;
            } else {
                phase = SUN;
            }
        } else {
            sun_hit = h.tri >= 0 ? h.tri : -1;
            if (sun_first) sun0 = sun_hit;
        }
        if (sun_hit != -2) {  // SUN (Raytracing.cl:115-137)
            rtm_f3 sunLight = rtm_v3(0, 0, 0);
            const Mat cm = load_mat(S.mat, __float_as_int(S.tri_shade[tri].w));
            if (sun_hit < 0 && cm.type != 3) sunLight = rtm_v3(e3, e3, e3);
            if (sun_hit >= 0) {
                const Mat sm = load_mat(S.mat, __float_as_int(S.tri_shade[sun_hit].w));
                if (sm.type == 3) sunLight = rtm_scale(sm.color, e3);
            }
            const rtm_f3 envLight = rtm_scale(sample_ibl_if<false>(S, C, Bd, e4, c), e4);
            so = rtm_mul(so, rtm_add(sunLight, envLight));
            finish = true;
        }
        if (finish) {
            acc = rtm_add(acc, so);
            ++s;
            if (s >= slim) {
                finish_ray();
            } else {
                tri = tc; j = 0;
                so = rtm_v3(1, 1, 1);
                phase = PREP;
            }
        }
    }
}

// rt_camera_rays*: ray i of the frame of C's camera -- genCameraRay's direction, the camera's position, and the
// seeds the render gives pixel i (Raytracing.cl:176-177)
__global__ void __launch_bounds__(256) camera_rays_kernel(const LaunchConst* __restrict__ lconst, int W, int npix,
                                                          int first, unsigned count, float4* __restrict__ rays) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const LaunchConst& C = *lconst;
    const int i = first + (int)t;
    const rtm_f3 d = camera_dir(C, W, i);
    rays[2 * (size_t)t] = make_float4(d.x, d.y, d.z, C.position.x);
    rays[2 * (size_t)t + 1] = make_float4(C.position.y, C.position.z, __uint_as_float((uint32_t)(i % npix)),
                                          __uint_as_float((uint32_t)(i / npix)));
}

}  // namespace

// the scene as the radiance kernel walks it (the plain form of launch_query: no persistent-grid overflow buffer,
// the whole FAST stack in LDS) and the largest block <= `block` whose stack fits; 0: none does
int radiance_fit(const DevScene& sc, int trav, int block, DevScene* out) {
    DevScene s2 = sc;
    s2.stack_lds = sc.depth > 0 ? sc.depth : 1;
    s2.stack_ovf = nullptr;
    while (block > 64 && stack_lds_bytes(s2, trav, block) > 64 * 1024) block /= 2;
    if (stack_lds_bytes(s2, trav, block) > 64 * 1024) return 0;
    if (out) *out = s2;
    return block;
}

size_t radiance_work_bytes() { return kRadConstOffset + sizeof(LaunchConst); }

bool radiance_fits(const DevScene& sc, int traversal, int block) {
    return radiance_fit(sc, traversal == TRAV_REF ? TRAV_REF : TRAV_FAST, block, nullptr) != 0;
}

hipError_t launch_radiance(const DevScene& sc, int traversal, const float4* rays, float4* state, int64_t n,
                           const RadianceOptions& q, void* work, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!rays || !state || !work) return hipErrorInvalidValue;
    const int trav = traversal == TRAV_REF ? TRAV_REF : TRAV_FAST;
    DevScene s2;
    const int block = radiance_fit(sc, trav, q.block, &s2);
    if (block == 0) return hipErrorInvalidValue;
    const size_t lds = stack_lds_bytes(s2, trav, block);
    const void* fn = trav == TRAV_REF ? (const void*)radiance_kernel<TRAV_REF> : (const void*)radiance_kernel<TRAV_FAST>;
    hipError_t e = hipSuccess;
    const int64_t resident = resident_blocks(fn, block, lds, q.max_waves, &e);
    if (e != hipSuccess) return e;
    int64_t grid = std::min<int64_t>((n + block - 1) / block, resident);
    if (q.grid_cap > 0) grid = std::min<int64_t>(grid, q.grid_cap);
    if (grid < 1) return hipErrorInvalidValue;
    unsigned* counter = static_cast<unsigned*>(work);
    LaunchConst* lc = reinterpret_cast<LaunchConst*>(static_cast<char*>(work) + kRadConstOffset);
    e = hipMemsetAsync(counter, 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    // the sun vector and the IBL's rotations; the camera fields are unused: a finite camera of width 1
    FrameParams fp{};
    fp.cam[6] = 1.0f;
    fp.cam[9] = 1.0f;
    std::memcpy(fp.env, q.env, sizeof fp.env);
    hipLaunchKernelGGL(make_const_kernel, dim3(1), dim3(64), 0, stream, fp, lc);
    // rays a wave reserves per atomic: launch_query's rule
    const int64_t waves = grid * (block / 64);
    unsigned chunk = (unsigned)std::min<int64_t>(512, std::max<int64_t>(64, n / waves / 4 / 64 * 64));
    unsigned un = (unsigned)n;
    int spp = q.spp, maxb = q.max_bounce, flags = q.flags;
    float e3 = q.env[3], e4 = q.env[4];
    const LaunchConst* clc = lc;
    void* args[] = {&s2, &rays, &state, &un, &spp, &maxb, &e3, &e4, &flags, &chunk, &counter, &clc};
    return hipLaunchKernel(fn, dim3((unsigned)grid), dim3((unsigned)block), args, lds, stream);
}

hipError_t launch_camera_rays(const float cam[10], int64_t npix, int64_t first, int64_t count, float4* rays,
                              void* work, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    if (!rays || !work) return hipErrorInvalidValue;
    LaunchConst* lc = reinterpret_cast<LaunchConst*>(static_cast<char*>(work) + kRadConstOffset);
    FrameParams fp{};
    std::memcpy(fp.cam, cam, sizeof fp.cam);
    hipLaunchKernelGGL(make_const_kernel, dim3(1), dim3(64), 0, stream, fp, lc);
    const unsigned grid = (unsigned)((count + 255) / 256);
    hipLaunchKernelGGL(camera_rays_kernel, dim3(grid), dim3(256), 0, stream, (const LaunchConst*)lc, (int)cam[6],
                       (int)npix, (int)first, (unsigned)count, rays);
    return hipGetLastError();
}

}  // namespace rt
