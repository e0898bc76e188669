// Lens frames (rt_lens_radiance*, rt_lens_rays*, rt_radiance_resolve_device, include/rt_api.h): a frame whose every
// sample goes down a camera ray of its own -- lens_ray(cam, lens, i, s), a box-filter jitter of the pixel and a thin
// lens -- generated on the device and summed into the pixel's 32-byte state record.  A translation unit of its own,
// like rt_radiance.hip: the instantiations below join no other module, so the code objects of every other kernel are
// what they were without it.
//
// The contract: a pixel's record is that of one fresh rt_radiance query per sample, of the ray
// lens_ray(i, s) at spp = 1, each starting from the seeds the one before left, the sums added in order.  The loop
// below is radiance_kernel's with one step more: at the start of every sample the lane evaluates its ray and enters
// PRIMARY, so the first hit is the sample's own and nothing is cached from sample to sample.
#include "rt_device.h"

namespace rt {

namespace {

// bits of lens_radiance_kernel's `flags`: radiance_kernel's
constexpr int kLensResume = 1;      // RT_RADIANCE_RESUME: sum, n and the seeds are read from the record
constexpr int kLensSunSkip = 2;     // FrameParams::sun_skip, as check_frame makes it
constexpr int kLensFixedPoint = 4;  // FrameParams::fixed_point; the degenerate lens only (launch_lens_radiance)
constexpr int kLensSunCache = 8;    // FrameParams::sun_cache; the degenerate lens only

constexpr int GEN = 64;   // the lane's next sample has no ray yet (beside PRIMARY / PREP / BOUNCE / SUN / FETCH)
static_assert(GEN != FETCH && GEN != PRIMARY && GEN != PREP && GEN != BOUNCE && GEN != SUN, "a phase of its own");

// what the kernels get of an rt_lens and the frame: wave-uniform
struct LensArgs {
    float jitter, aperture, focus;
    uint32_t hseed;   // h(seed)
    int W, npix, first;
};

// the uniforms' hash (rt_api.h): uint32 arithmetic modulo 2^32
__host__ __device__ __forceinline__ uint32_t lens_hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float lens_uniform(uint32_t base, uint32_t k) {
    return (float)(lens_hash(base + k) >> 8) * 5.9604644775390625e-08f;   // 24 bits * 2^-24: exact, in [0, 1)
}

// lens_ray(cam, lens, i, s) of rt_api.h, operation by operation; the one evaluation, of lens_rays_kernel and of the
// render loop.  camera_dir's values (rt_device.h) with the jitter added to the pixel's coordinates before the fmaf;
// the lens in the camera's local frame, before the three rotations.
__device__ __forceinline__ void lens_ray(const LaunchConst& C, const LensArgs& L, int i, uint32_t s, rtm_f3* o,
                                         rtm_f3* dir) {
    const uint32_t base = lens_hash(L.hseed ^ (uint32_t)i) + 4u * s;
    const int pixelY = (i + 1) % L.W;
    const int pixelX = (i - pixelY) / L.W;
    const float jx = (lens_uniform(base, 0) - 0.5f) * L.jitter;
    const float jy = (lens_uniform(base, 1) - 0.5f) * L.jitter;
    const rtm_f3 pc = rtm_v3(fmaf((float)pixelY + jx, C.pas, -0.5f), 0.0f, fmaf(-((float)pixelX + jy), C.pas, 0.5f));
    rtm_f3 d = dev_normalize(rtm_sub(rtm_add(C.position, pc), C.focal));
    if (L.aperture == 0.0f) {   // the pinhole
        d = rtm_rot_apply(C.cam_rx, d);
        d = rtm_rot_apply(C.cam_ry, d);
        *dir = rtm_rot_apply(C.cam_rz, d);
        *o = C.position;
        return;
    }
    const float r = dev_sqrt(lens_uniform(base, 2)) * L.aperture;
    float sn, cs;
    rtm_sincos(6.2831855f * lens_uniform(base, 3), &sn, &cs);
    rtm_f3 l = rtm_v3(r * cs, 0.0f, r * sn);
    const float t = L.focus / d.y;
    d = dev_normalize(rtm_sub(rtm_scale(d, t), l));
    d = rtm_rot_apply(C.cam_rx, d);
    d = rtm_rot_apply(C.cam_ry, d);
    *dir = rtm_rot_apply(C.cam_rz, d);
    l = rtm_rot_apply(C.cam_rx, l);
    l = rtm_rot_apply(C.cam_ry, l);
    l = rtm_rot_apply(C.cam_rz, l);
    *o = rtm_add(C.position, l);
}

// Persistent wave64, radiance_kernel's state machine with GEN in front of every sample.  A job is a pixel of the
// call's slice: one atomic reserves `chunk` consecutive pixels for the wave (query_walk_kernel's hand-out), its
// refills hand them out in order.  A refill of a fresh call reads nothing (the seeds are the pixel's index); on
// resume it reads the record's two float4, of which tri and k are dropped: every sample traces its own ray, so no
// index comes from the caller's data.
// The traversal is trace<>, as radiance_kernel uses it.  sun_skip carries over (it does not depend on the ray);
// fixed_point and sun_cache are set by the launch for the degenerate lens alone, whose samples share one ray.
// amdgpu_waves_per_eu(5): the register allocator keeps the kernel within 96 VGPRs, radiance_kernel's 5 waves per
// SIMD (left alone, the scheduler spreads the ray's evaluation over 102).
template <int TRAV>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5)))
lens_radiance_kernel(DevScene S, LensArgs L, float4* __restrict__ state, unsigned n, int spp, int maxB, float e3, float e4,
                     int flags, unsigned chunk, unsigned* __restrict__ counter, const LaunchConst* __restrict__ lconst) {
    extern __shared__ __attribute__((aligned(16))) int lds_stack[];
    const int B = blockDim.x;
    int* stk = lds_stack + threadIdx.x;
    const LaneStack lst = lane_stack(S, lds_stack);
    Cnt c{};
    const LaunchConst& C = *lconst;   // uniform: the camera, the sun vector and the IBL's rotations
    const int lane = threadIdx.x & 63;
    const bool resume = (flags & kLensResume) != 0;
    const bool sun_skip = TRAV == TRAV_FAST && (flags & kLensSunSkip) != 0;
    const bool fixed_point = TRAV == TRAV_FAST && (flags & kLensFixedPoint) != 0;
    const bool sun_cache = TRAV == TRAV_FAST && (flags & kLensSunCache) != 0;

    int phase = FETCH;
    unsigned idx = 0;
    uint32_t seed0 = 0, seed1 = 0;
    rtm_f3 co = rtm_v3(0, 0, 0), cd = rtm_v3(0, 0, 1);   // the sample's ray
    float kc = 1000.0f;                                  // its hit
    int tc = -1;
    rtm_f3 so = rtm_v3(1, 1, 1);
    float k = 1000.0f;
    int tri = -1, j = 0;
    rtm_f3 Bo = rtm_v3(0, 0, 0), Bd = rtm_v3(0, 0, 0);
    rtm_f3 acc = rtm_v3(0, 0, 0);
    int s = 0, slim = 0;
    int sun0 = -2;   // the first bounce's shadow-ray hit (-1 = miss; -2 = not traced yet)
    bool dry = false;                  // wave-uniform: the slice is handed out
    unsigned wnext = 0, wend = 0;      // the wave's run of pixels not yet handed to a lane (wave-uniform)

    auto finish_pixel = [&]() __attribute__((always_inline)) {
        state[2 * (size_t)idx] = make_float4(acc.x, acc.y, acc.z, kc);
        state[2 * (size_t)idx + 1] =
            make_float4(__uint_as_float(seed0), __uint_as_float(seed1), __int_as_float(tc), __int_as_float(s));
        phase = FETCH;
    };

    while (true) {
        if (TRAV == TRAV_FAST && S.nbrute > 0) wave_lds_sync();   // (brute force: the next trace rewrites the wave's tables)
        const unsigned long long need = __ballot(phase == FETCH);
        if (!dry && need) {
            const unsigned cnt = (unsigned)__popcll(need), left = wend - wnext;
            const unsigned r = lane_prefix(need, 0u);
            unsigned my = wnext + r;
            bool valid = true;
            if (left < cnt) {
                const int first = __ffsll((long long)need) - 1;
                unsigned base = 0;
                if (lane == first) base = atomicAdd(counter, chunk);
                base = (unsigned)__shfl((int)base, first, 64);
                const unsigned rb = min(base, n), re = min(base + chunk, n);   // the new run, cut at the slice's end
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
                sun0 = -2;
                if (resume) {
                    const float4 u = state[2 * (size_t)idx], v = state[2 * (size_t)idx + 1];
                    acc = rtm_v3(u.x, u.y, u.z);
                    seed0 = __float_as_uint(v.x);
                    seed1 = __float_as_uint(v.y);
                    s = __float_as_int(v.w);
                } else {
                    const int i = L.first + (int)idx;
                    acc = rtm_v3(0, 0, 0);
                    seed0 = (uint32_t)(i % L.npix);
                    seed1 = (uint32_t)(i / L.npix);
                    s = 0;
                }
                slim = (int)((unsigned)s + (unsigned)spp);
                phase = GEN;
            }
        }
        if (__ballot(phase != FETCH) == 0) {
            if (dry) break;
            continue;
        }
        if (phase == FETCH) continue;

        if (phase == GEN) {   // sample s of the pixel: its own ray, then its own first hit
            lens_ray(C, L, L.first + (int)idx, (uint32_t)s, &co, &cd);
            phase = PRIMARY;
        }

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
                // the degenerate lens: a sample that ends at its first loop head drew no random number, and the next
                // sample's ray is this ray: every later sample of the call is this sample again, added in order
                if (fixed_point && j == 0)
                    for (; s < slim; ++s) acc = rtm_add(acc, so);
                if (s >= slim) finish_pixel();
                else phase = GEN;
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
            if (s >= slim) finish_pixel();
            else phase = GEN;
        }
    }
}

// rt_lens_rays*: ray (pixel first + t / nsamples, sample sample0 + t % nsamples) in rt_camera_rays' layout; the seed
// words are the pixel's frame seeds, the same for each of its samples
__global__ void __launch_bounds__(256) lens_rays_kernel(const LaunchConst* __restrict__ lconst, LensArgs L, int sample0,
                                                        unsigned nsamples, unsigned total, float4* __restrict__ rays) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int i = L.first + (int)(t / nsamples);
    rtm_f3 o, d;
    lens_ray(*lconst, L, i, (uint32_t)sample0 + t % nsamples, &o, &d);
    rays[2 * (size_t)t] = make_float4(d.x, d.y, d.z, o.x);
    rays[2 * (size_t)t + 1] = make_float4(o.y, o.z, __uint_as_float((uint32_t)(i % L.npix)),
                                          __uint_as_float((uint32_t)(i / L.npix)));
}

// rt_radiance_resolve_device: Raytracing.cl:211-220 on a record, fmax(fmin(sum / (float)n, 1), 0) -- NaN goes to 1
__global__ void __launch_bounds__(256) resolve_kernel(const float4* __restrict__ state, unsigned n,
                                                      float* __restrict__ rgb) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const float4 u = state[2 * (size_t)t];
    const float cnt = (float)__float_as_int(state[2 * (size_t)t + 1].w);
    rgb[3 * (size_t)t] = fmaxf(fminf(u.x / cnt, 1.0f), 0.0f);
    rgb[3 * (size_t)t + 1] = fmaxf(fminf(u.y / cnt, 1.0f), 0.0f);
    rgb[3 * (size_t)t + 2] = fmaxf(fminf(u.z / cnt, 1.0f), 0.0f);
}

LensArgs lens_args(const LensOptions& q, const float cam[10], int64_t npix, int64_t first) {
    LensArgs L;
    L.jitter = q.jitter;
    L.aperture = q.aperture;
    L.focus = q.focus;
    L.hseed = lens_hash(q.seed);
    L.W = (int)cam[6];
    L.npix = (int)npix;
    L.first = (int)first;
    return L;
}

LaunchConst* lens_const(const float cam[10], const float* env, void* work, hipStream_t stream) {
    LaunchConst* lc = reinterpret_cast<LaunchConst*>(static_cast<char*>(work) + kRadConstOffset);
    FrameParams fp{};
    std::memcpy(fp.cam, cam, sizeof fp.cam);
    if (env) std::memcpy(fp.env, env, sizeof fp.env);
    hipLaunchKernelGGL(make_const_kernel, dim3(1), dim3(64), 0, stream, fp, lc);
    return lc;
}

}  // namespace

hipError_t launch_lens_radiance(const DevScene& sc, int traversal, const float cam[10], int64_t npix, int64_t first,
                                int64_t count, float4* state, const LensOptions& lens, const RadianceOptions& q,
                                void* work, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    if (!state || !work) return hipErrorInvalidValue;
    const int trav = traversal == TRAV_REF ? TRAV_REF : TRAV_FAST;
    DevScene s2;
    const int block = radiance_fit(sc, trav, q.block, &s2);
    if (block == 0) return hipErrorInvalidValue;
    const size_t lds = stack_lds_bytes(s2, trav, block);
    const void* fn = trav == TRAV_REF ? (const void*)lens_radiance_kernel<TRAV_REF>
                                      : (const void*)lens_radiance_kernel<TRAV_FAST>;
    hipError_t e = hipSuccess;
    const int64_t resident = resident_blocks(fn, block, lds, q.max_waves, &e);
    if (e != hipSuccess) return e;
    int64_t grid = std::min<int64_t>((count + block - 1) / block, resident);
    if (q.grid_cap > 0) grid = std::min<int64_t>(grid, q.grid_cap);
    if (grid < 1) return hipErrorInvalidValue;
    unsigned* counter = static_cast<unsigned*>(work);
    e = hipMemsetAsync(counter, 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    const LaunchConst* clc = lens_const(cam, q.env, work, stream);   // the real camera, the sun, the IBL's rotations
    // pixels a wave reserves per atomic: launch_radiance's rule
    const int64_t waves = grid * (block / 64);
    unsigned chunk = (unsigned)std::min<int64_t>(512, std::max<int64_t>(64, count / waves / 4 / 64 * 64));
    LensArgs L = lens_args(lens, cam, npix, first);
    unsigned un = (unsigned)count;
    int spp = q.spp, maxb = q.max_bounce, flags = q.flags;
    // the shortcuts that rest on every sample sharing one ray: the degenerate lens only
    if (lens.jitter != 0.0f || lens.aperture != 0.0f) flags &= ~(kLensFixedPoint | kLensSunCache);
    float e3 = q.env[3], e4 = q.env[4];
    void* args[] = {&s2, &L, &state, &un, &spp, &maxb, &e3, &e4, &flags, &chunk, &counter, &clc};
    return hipLaunchKernel(fn, dim3((unsigned)grid), dim3((unsigned)block), args, lds, stream);
}

hipError_t launch_lens_rays(const float cam[10], int64_t npix, int64_t first, int64_t count, int sample0,
                            int nsamples, const LensOptions& lens, float4* rays, void* work, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    if (!rays || !work || nsamples < 1 || count * nsamples >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const LaunchConst* lc = lens_const(cam, nullptr, work, stream);
    const unsigned total = (unsigned)(count * nsamples);
    const unsigned grid = (total + 255) / 256;
    hipLaunchKernelGGL(lens_rays_kernel, dim3(grid), dim3(256), 0, stream, lc, lens_args(lens, cam, npix, first),
                       sample0, (unsigned)nsamples, total, rays);
    return hipGetLastError();
}

hipError_t launch_resolve(const float4* state, int64_t n, float* rgb, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!state || !rgb) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(resolve_kernel, dim3(grid), dim3(256), 0, stream, state, (unsigned)n, rgb);
    return hipGetLastError();
}

}  // namespace rt
