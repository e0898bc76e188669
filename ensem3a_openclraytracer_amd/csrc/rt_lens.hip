// Lens frames (rt_lens_radiance*, rt_lens_rays*, rt_radiance_resolve_device, include/rt_api.h): a frame whose every
// sample goes down a camera ray of its own -- lens_ray(cam, lens, i, s), a box-filter jitter of the pixel and a thin
// lens -- generated on the device and summed into the pixel's 32-byte state record.  A translation unit of its own,
// like rt_radiance.hip: the instantiations below join no other module, so the code objects of every other kernel are
// what they were without it.  Lens frames inside an accumulation (rt_accum_begin_lens*) are further
// instantiations of the same loop -- the tile and listed job mappings -- with three small kernels of their own: the
// records a begin leaves, the centre-hit pass of the guides, and the guides from its buffer.
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

// How a job index t of lens_radiance_kernel becomes a record slot p and a frame pixel i:
//   kMapContig  p = t, i = first + t: rt_lens_radiance's slice of the frame;
//   kMapTile    p = t, i = tile_pixel(p): the tile-packed state of an accumulation (rt_accum_add on a lens frame);
//   kMapListed  p = list[t], i = tile_pixel(p), the job count read from the device word the compaction wrote
//               (rt_accum_add_selected; a full add once the counts differ).
// A tile job whose pixel is padding of a partial last row (i >= npix) is dropped at the refill, as is a listed p that
// is no pixel of the tile: no index is used unchecked.
constexpr int kMapContig = 0, kMapTile = 1, kMapListed = 2;
struct LensJobs {   // what the tile and listed mappings add to LensArgs: wave-uniform (kMapContig reads none of it)
    int row0, row_step;
    unsigned nloc;            // records in the state
    const uint32_t* list;     // kMapListed: tile pixels, ascending
    const uint32_t* count;    // ... and how many
};

// pixel p of the tile of rows row0, row0 + row_step, ... -> the frame's pixel; false: padding of a partial last row
__device__ __forceinline__ bool lens_tile_pixel(unsigned p, int W, int row0, int row_step, int npix, int* i) {
    const unsigned krow = p / (unsigned)W;
    const long long i64 = ((long long)row0 + (long long)krow * row_step) * W + (long long)(p - krow * (unsigned)W);
    *i = (int)i64;
    return i64 < npix;   // (npix < 2^31: check_frame)
}

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
// index comes from the caller's data.  MAP (above): the tile and listed mappings always resume -- an accumulation's
// records are initialised by its begin (lens_init_kernel) -- and carry the pixel i in a register from the refill, so
// that no sample pays the mapping's division.
// The traversal is trace<>, as radiance_kernel uses it.  sun_skip carries over (it does not depend on the ray);
// fixed_point and sun_cache are set by the launch for the degenerate lens alone, whose samples share one ray.
// amdgpu_waves_per_eu(5): the register allocator keeps the kernel within 96 VGPRs, radiance_kernel's 5 waves per
// SIMD (left alone, the scheduler spreads the ray's evaluation over 102).
template <int TRAV, int MAP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5)))
lens_radiance_kernel(DevScene S, LensArgs L, float4* __restrict__ state, unsigned n_, int spp, int maxB, float e3, float e4,
                     int flags, unsigned chunk, unsigned* __restrict__ counter, const LaunchConst* __restrict__ lconst,
                     LensJobs J) {
    extern __shared__ __attribute__((aligned(16))) int lds_stack[];
    const int B = blockDim.x;
    int* stk = lds_stack + threadIdx.x;
    const LaneStack lst = lane_stack(S, lds_stack);
    Cnt c{};
    const LaunchConst& C = *lconst;   // uniform: the camera, the sun vector and the IBL's rotations
    const int lane = threadIdx.x & 63;
    const bool resume = MAP != kMapContig || (flags & kLensResume) != 0;
    // the jobs: the launch's count, or the list's length (never past the tile: list holds nloc words)
    const unsigned n = MAP == kMapListed ? min(*J.count, J.nloc) : n_;
    const bool sun_skip = TRAV == TRAV_FAST && (flags & kLensSunSkip) != 0;
    const bool fixed_point = TRAV == TRAV_FAST && (flags & kLensFixedPoint) != 0;
    const bool sun_cache = TRAV == TRAV_FAST && (flags & kLensSunCache) != 0;

    int phase = FETCH;
    unsigned idx = 0;   // the lane's record slot p
    int pix = 0;        // ... and its frame pixel i (kMapContig: first + idx, not kept)
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
            if (MAP == kMapListed && phase == FETCH && valid) {
                my = J.list[my];
                valid = my < J.nloc;
            }
            if (MAP != kMapContig && phase == FETCH && valid)
                valid = lens_tile_pixel(my, L.W, J.row0, J.row_step, L.npix, &pix);
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
            lens_ray(C, L, MAP == kMapContig ? L.first + (int)idx : pix, (uint32_t)s, &co, &cd);
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

// rt_accum_begin_lens*: the records a tile's pixels start from -- sum 0, n 0, the frame's seeds (i % npix, i / npix),
// the hit of a miss -- so that every add resumes (lens_state of KernelLauncher.py makes the same words)
__global__ void __launch_bounds__(256) lens_init_kernel(float4* __restrict__ state, unsigned nloc, int W, int row0,
                                                        int row_step, int npix) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nloc) return;
    int i;
    (void)lens_tile_pixel(p, W, row0, row_step, npix, &i);   // (a padding pixel's record is never read by a job)
    state[2 * (size_t)p] = make_float4(0.0f, 0.0f, 0.0f, 1000.0f);
    state[2 * (size_t)p + 1] = make_float4(__uint_as_float((uint32_t)(i % npix)), __uint_as_float((uint32_t)(i / npix)),
                                           __int_as_float(-1), __int_as_float(0));
}

// The centre-hit pass of a lens accumulation's guides: genCameraRay(i) of every tile pixel -- camera_dir from the
// camera's position, rt_camera_rays' ray -- traced as rt_trace's plain form traces it (query_plain_kernel: one thread
// per ray, trace<>, the whole stack in LDS), (k, tri) as a record's PRIMARY step stores them; a padding pixel a miss.
template <int TRAV>
__global__ void __launch_bounds__(256) lens_centre_kernel(DevScene S, const LaunchConst* __restrict__ lconst, int W,
                                                          int row0, int row_step, int npix, unsigned nloc,
                                                          float2* __restrict__ centre) {
    extern __shared__ int lds_stack[];
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nloc) return;
    int i;
    if (!lens_tile_pixel(p, W, row0, row_step, npix, &i)) {
        centre[p] = make_float2(1000.0f, __int_as_float(-1));
        return;
    }
    Cnt c{};
    const LaunchConst& C = *lconst;
    const Hit h = trace<TRAV, false>(S, S.nodes, S.tri_fast, C.position, camera_dir(C, W, i), lds_stack + threadIdx.x,
                                     blockDim.x, lane_stack(S, lds_stack), c);
    centre[p] = h.tri >= 0 ? make_float2(h.k, __int_as_float(h.tri)) : make_float2(1000.0f, __int_as_float(-1));
}

// A pixel's guides (rt_api.h: G0 = n | k, G1 = P | f, G2 = a | m) from the first hit (tc, kc) of its camera ray and
// its sample count s; a miss keeps the pattern a fresh Guide has.  guides_kernel's evaluation (rt_denoise.hip),
// operation by operation, restated here and not shared: sharing it through a header changes guides_kernel's
// instruction schedule, and every code object but this one stays what it was.
struct Guide {
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    float4 g1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0));
    float4 g2 = make_float4(1.0f, 1.0f, 1.0f, __int_as_float(-1));
};
__device__ __forceinline__ void guide_of_hit(Guide& g, const LaunchConst& C, const float4* __restrict__ tri_shade,
                                             const float* __restrict__ mat, int ntri, int nmat, int W, int i, int tc,
                                             float kc, int s) {
    if (tc < 0 || tc >= ntri) return;
    const float4 sh = tri_shade[tc];
    const int m = __float_as_int(sh.w);
    const rtm_f3 d = camera_dir(C, W, i);
    g.g0 = make_float4(sh.x, sh.y, sh.z, kc);
    g.g1.x = C.position.x + d.x * kc;
    g.g1.y = C.position.y + d.y * kc;
    g.g1.z = C.position.z + d.z * kc;
    g.g2.w = __int_as_float(m);
    if (m >= 0 && m < nmat) {
        const int type = (int)mat[kMatF * m];
        if (type == 1 || type == 2) {
            g.g1.w = __int_as_float(s);
            g.g2.x = rtm_fmax(mat[kMatF * m + 1], 0.01f);
            g.g2.y = rtm_fmax(mat[kMatF * m + 2], 0.01f);
            g.g2.z = rtm_fmax(mat[kMatF * m + 3], 0.01f);
        }
    }
}

// rt_accum_guides of a lens accumulation: guides_kernel (rt_denoise.hip) with the first hit out of the centre-hit
// buffer -- a lens record's k, tri are its last sample's -- and the count out of the state
__global__ void __launch_bounds__(256) lens_guides_kernel(const float4* __restrict__ state,
                                                          const float2* __restrict__ centre,
                                                          const float4* __restrict__ tri_shade,
                                                          const float* __restrict__ mat, int ntri, int nmat,
                                                          unsigned nloc, int W, int row0, int row_step, int npix,
                                                          const LaunchConst* __restrict__ lconst,
                                                          float4* __restrict__ out) {
    const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nloc) return;
    Guide g;
    int i;
    if (lens_tile_pixel(p, W, row0, row_step, npix, &i)) {
        const float2 h = centre[p];
        guide_of_hit(g, *lconst, tri_shade, mat, ntri, nmat, W, i, __float_as_int(h.y), h.x,
                     __float_as_int(state[2 * (size_t)p + 1].w));
    }
    out[3 * (size_t)p + 0] = g.g0;
    out[3 * (size_t)p + 1] = g.g1;
    out[3 * (size_t)p + 2] = g.g2;
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

// the render loop over `count` jobs under mapping `map` (count: the most jobs a listed launch can have -- its grid and
// its runs are sized for it, the kernel reads the length)
hipError_t launch_lens_jobs(const DevScene& sc, int traversal, const float cam[10], int64_t npix, int64_t first,
                            int64_t count, int map, LensJobs J, float4* state, const LensOptions& lens,
                            const RadianceOptions& q, void* work, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    if (!state || !work) return hipErrorInvalidValue;
    const int trav = traversal == TRAV_REF ? TRAV_REF : TRAV_FAST;
    DevScene s2;
    const int block = radiance_fit(sc, trav, q.block, &s2);
    if (block == 0) return hipErrorInvalidValue;
    const size_t lds = stack_lds_bytes(s2, trav, block);
    const void* const fns[2][3] = {
        {(const void*)lens_radiance_kernel<TRAV_FAST, kMapContig>, (const void*)lens_radiance_kernel<TRAV_FAST, kMapTile>,
         (const void*)lens_radiance_kernel<TRAV_FAST, kMapListed>},
        {(const void*)lens_radiance_kernel<TRAV_REF, kMapContig>, (const void*)lens_radiance_kernel<TRAV_REF, kMapTile>,
         (const void*)lens_radiance_kernel<TRAV_REF, kMapListed>}};
    if (map < kMapContig || map > kMapListed) return hipErrorInvalidValue;
    const void* fn = fns[trav == TRAV_REF][map];
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
    void* args[] = {&s2, &L, &state, &un, &spp, &maxb, &e3, &e4, &flags, &chunk, &counter, &clc, &J};
    return hipLaunchKernel(fn, dim3((unsigned)grid), dim3((unsigned)block), args, lds, stream);
}

LensJobs lens_jobs(const FrameParams& fp, const uint32_t* list, const uint32_t* count) {
    LensJobs J{};
    J.row0 = fp.row0;
    J.row_step = fp.row_step;
    J.nloc = (unsigned)fp.nloc;
    J.list = list;
    J.count = count;
    return J;
}

// the camera ray's kernels run in blocks of 256 or, where the stack of one does not fit, the largest that does
template <typename F>
hipError_t launch_lens_centre_(F fn, const DevScene& s2, int block, size_t lds, const LaunchConst* lc,
                               const FrameParams& fp, float2* centre, hipStream_t stream) {
    hipLaunchKernelGGL(fn, dim3((unsigned)((fp.nloc + block - 1) / block)), dim3((unsigned)block), lds, stream, s2, lc,
                       fp.width, fp.row0, fp.row_step, (int)fp.npix, (unsigned)fp.nloc, centre);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_lens_radiance(const DevScene& sc, int traversal, const float cam[10], int64_t npix, int64_t first,
                                int64_t count, float4* state, const LensOptions& lens, const RadianceOptions& q,
                                void* work, hipStream_t stream) {
    return launch_lens_jobs(sc, traversal, cam, npix, first, count, kMapContig, LensJobs{}, state, lens, q, work, stream);
}

hipError_t launch_lens_accum_init(const FrameParams& fp, float4* state, hipStream_t stream) {
    if (fp.nloc <= 0) return hipSuccess;
    if (!state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lens_init_kernel, dim3((unsigned)((fp.nloc + 255) / 256)), dim3(256), 0, stream, state,
                       (unsigned)fp.nloc, fp.width, fp.row0, fp.row_step, (int)fp.npix);
    return hipGetLastError();
}

hipError_t launch_lens_accum(const DevScene& sc, int traversal, const FrameParams& fp, float4* state,
                             const uint32_t* list, const uint32_t* count, const LensOptions& lens,
                             const RadianceOptions& q, void* work, hipStream_t stream) {
    if (list && !count) return hipErrorInvalidValue;
    return launch_lens_jobs(sc, traversal, fp.cam, fp.npix, 0, fp.nloc, list ? kMapListed : kMapTile,
                            lens_jobs(fp, list, count), state, lens, q, work, stream);
}

hipError_t launch_lens_centre(const DevScene& sc, int traversal, const FrameParams& fp, float2* centre, void* work,
                              hipStream_t stream) {
    if (fp.nloc <= 0) return hipSuccess;
    if (!centre || !work) return hipErrorInvalidValue;
    const int trav = traversal == TRAV_REF ? TRAV_REF : TRAV_FAST;
    DevScene s2;
    const int block = radiance_fit(sc, trav, 256, &s2);
    if (block == 0) return hipErrorInvalidValue;
    const size_t lds = stack_lds_bytes(s2, trav, block);
    const LaunchConst* lc = lens_const(fp.cam, nullptr, work, stream);
    return trav == TRAV_REF ? launch_lens_centre_(lens_centre_kernel<TRAV_REF>, s2, block, lds, lc, fp, centre, stream)
                            : launch_lens_centre_(lens_centre_kernel<TRAV_FAST>, s2, block, lds, lc, fp, centre, stream);
}

hipError_t launch_lens_guides(const DevScene& sc, const FrameParams& fp, const float4* state, const float2* centre,
                              void* work, float4* d_guides, hipStream_t stream) {
    if (fp.nloc <= 0) return hipSuccess;
    if (!state || !centre || !work || !d_guides) return hipErrorInvalidValue;
    const LaunchConst* lc = lens_const(fp.cam, nullptr, work, stream);
    hipLaunchKernelGGL(lens_guides_kernel, dim3((unsigned)((fp.nloc + 255) / 256)), dim3(256), 0, stream, state, centre,
                       sc.tri_shade, sc.mat, sc.ntri, sc.nmat, (unsigned)fp.nloc, fp.width, fp.row0, fp.row_step,
                       (int)fp.npix, lc, d_guides);
    return hipGetLastError();
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
