// Test hook rt_debug_fn (rt_debug.h): the shading and hit functions of rt_device.h -- the ones the render
// kernels call, from the same header -- evaluated one call per item on chosen inputs, so that the tests can
// compare each of them with the CPU oracle's function instead of through whole frames; and the clustered
// brute-force trace on the caller's rays (rt_debug_trace_clustered).  No render kernel lives here and none is
// changed by this file.
#include "../../include/rt_debug.h"
#include "rt_device.h"

namespace rt {

namespace {

static_assert(RT_FN_COUNT == kDebugFns, "debug_fn_in / debug_fn_out list every function");

__device__ __forceinline__ float ubits(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ rtm_f3 ld3(const float* p) { return rtm_v3(p[0], p[1], p[2]); }
__device__ __forceinline__ void st3(float* p, rtm_f3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

// camera / sun: the launch constants as make_const prepares them for the item's cam / env, then camera_dir
__global__ void debug_camera_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* x = in + debug_fn_in(RT_FN_CAMERA) * i;
    FrameParams F{};
    for (int k = 0; k < 10; ++k) F.cam[k] = x[k];
    F.width = (int)x[6];
    const LaunchConst C = make_const(F);
    st3(out + 3 * i, camera_dir(C, F.width, __float_as_int(x[10])));
}

__global__ void debug_sun_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* x = in + debug_fn_in(RT_FN_SUN) * i;
    FrameParams F{};
    F.cam[6] = 1.0f;
    F.cam[9] = 1.0f;
    for (int k = 0; k < 5; ++k) F.env[k] = x[k];
    st3(out + 3 * i, make_const(F).sun);
}

// hemisphere samplers: item i becomes triangle i of a synthetic scene (normal n, material 0 = type 1,
// material 1 = type 2) whose frames prep_frames_kernel then computes as it does for an uploaded scene
__global__ void debug_hemi_scene_kernel(const float* __restrict__ in, float4* __restrict__ tri_shade,
                                        float* __restrict__ mat, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * kMatF) mat[i] = i == 0 ? 1.0f : (i == kMatF ? 2.0f : 0.0f);
    if (i >= n) return;
    const float* x = in + debug_fn_in(RT_FN_HEMI) * i;
    tri_shade[i] = make_float4(x[0], x[1], x[2], __int_as_float(x[3] == 2.0f ? 1 : 0));
}

__global__ void debug_hemi_kernel(const float* __restrict__ in, const float4* __restrict__ tri_shade,
                                  const float4* __restrict__ frame, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* x = in + debug_fn_in(RT_FN_HEMI) * i;
    const rtm_f3 nrm = xyz(tri_shade[i]);
    const float4 f0 = frame[3 * i], f1 = frame[3 * i + 1], f2 = frame[3 * i + 2];
    float* o = out + debug_fn_out(RT_FN_HEMI) * i;
    for (int form = 0; form < 4; ++form) {
        uint32_t s0 = __float_as_uint(x[4]), s1 = __float_as_uint(x[5]);
        float inv = 0.0f;
        rtm_f3 d;
        if (form == 0) d = hemi_cosine(nrm, f0, f1, f2, &s0, &s1, &inv);
        else if (form == 1) d = hemi_uniform(nrm, f0, f1, f2, &s0, &s1, &inv);
        else d = hemi_sample(form == 2, nrm, f0, f1, f2, &s0, &s1, &inv);
        st3(o + 6 * form, d);
        o[6 * form + 3] = inv;
        o[6 * form + 4] = ubits(s0);
        o[6 * form + 5] = ubits(s1);
    }
}

__global__ void debug_ggx_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* x = in + debug_fn_in(RT_FN_GGX) * i;
    st3(out + 3 * i, brdf_ggx(ld3(x), x[3], ld3(x + 4), ld3(x + 7), ld3(x + 10)));
}

// the uploaded environment's texel-sum table (S.ibl_sum: ibl_sum_kernel's, at rt_set_env) through sample_ibl
__global__ void debug_ibl_kernel(DevScene S, const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* x = in + debug_fn_in(RT_FN_IBL) * i;
    FrameParams F{};
    F.cam[6] = 1.0f;
    F.cam[9] = 1.0f;
    const LaunchConst C = make_const(F);
    Cnt c{};
    st3(out + 6 * i, sample_ibl<false>(S, C, ld3(x), c));
    st3(out + 6 * i + 3, sample_ibl_if<false>(S, C, ld3(x), x[3], c));
}

// Moller-Trumbore on a record of DevScene::tri_geo's form (a.p | rank, e1 | index, e2 | 0), then dir, origin
template <bool FAST>
__global__ void debug_mt_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    static_assert(debug_fn_in(RT_FN_MT_REF) == 24 && debug_fn_in(RT_FN_MT_FAST) == 24, "six float4 per item");
    const float4* rec = reinterpret_cast<const float4*>(in) + 6 * i;
    const float* r = in + 24 * i + 12;
    const rtm_f3 d = ld3(r), o = ld3(r + 3);
    float k = 1000.0f;   // a miss of mt_test leaves k alone: MathLib.cl's output.k of a miss
    int rank = 0;
    bool hit;
    if (FAST) hit = mt_core(xyz(rec[0]), xyz(rec[1]), xyz(rec[2]), o, d, &k);
    else hit = mt_test(rec, 0, o, d, &k, &rank);
    out[2 * i] = hit ? 1.0f : 0.0f;
    out[2 * i + 1] = k;
}

__global__ void debug_box_ref_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* x = in + debug_fn_in(RT_FN_BOX_REF) * i;
    out[i] = ref_box(x + 6, ld3(x + 3), ld3(x)) ? 1.0f : 0.0f;
}

// the FAST walks' test of one box: the inverses as fast_init / trace_fast form them, slab, box_hit
__global__ void debug_box_fast_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* x = in + debug_fn_in(RT_FN_BOX_FAST) * i;
    const rtm_f3 d = ld3(x), o = ld3(x + 3);
    const float ix = dev_recip(d.x), iy = dev_recip(d.y), iz = dev_recip(d.z);
    float tmin, tmax;
    slab(x[6], x[9], x[7], x[10], x[8], x[11], o, ix, iy, iz, tmin, tmax);
    out[3 * i] = box_hit(tmin, tmax, x[12]) ? 1.0f : 0.0f;
    out[3 * i + 1] = tmin;
    out[3 * i + 2] = tmax;
}

// rt_debug_trace_clustered: the clustered product trace -- trace_brute_compact<false, true> itself, the function
// render_kernel's BRUTE == 3 instantiations call -- on the caller's rays, one ray per lane.  The block stages what
// that trace reads from LDS as render_kernel's prologue does: the waves' areas (BRUTE_WAVE_LDS each) | the records'
// copy (stage_mt_records, stride 3) | the slots of brute_cbox, with the shell's rows behind them at boxrec + S.shell.
// Lanes past n leave after the staging, so the last wave of a launch is a partial one, as in a frame's tail.
__global__ void __launch_bounds__(256) debug_trace_clustered_kernel(DevScene S, const float* __restrict__ rays,
                                                                    float* __restrict__ out, int64_t n) {
    extern __shared__ __attribute__((aligned(16))) int lds_stack[];
    const int B = blockDim.x;
    float4* lr = reinterpret_cast<float4*>(reinterpret_cast<char*>(lds_stack) + (B / 64) * BRUTE_WAVE_LDS);
    float4* lc = lr + 3 * S.nbrute;
    stage_mt_records(lr, S.brute, S.nbrute);
    for (int q = threadIdx.x; q < 2 * S.ncslot; q += B) lc[q] = S.brute_cbox[q];
    if (S.shell)
        for (int q = threadIdx.x; q < 2 * kShellRows; q += B) lc[S.shell + q] = S.brute_cbox[S.shell + kShellRowF4 + q];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * B + threadIdx.x;
    if (i >= n) return;
    const float* r = rays + 6 * i;
    Cnt c{};
    const Hit h = trace_brute_compact<false, true>(S, ld3(r + 3), ld3(r), reinterpret_cast<char*>(lds_stack) +
                                                                          (threadIdx.x >> 6) * BRUTE_WAVE_LDS,
                                                   lr, 3u, c, 1, lc);
    out[2 * i] = h.k;
    out[2 * i + 1] = __int_as_float(h.tri);
}

}  // namespace

// What debug_trace_clustered_kernel stages (above); brute_lds_bytes' terms without the shading tables
static size_t debug_clustered_lds_bytes(const DevScene& sc, int block) {
    return (size_t)(block / 64) * BRUTE_WAVE_LDS + (size_t)sc.nbrute * 48 + (size_t)sc.ncslot * 32 +
           (sc.shell ? (size_t)kShellRows * 32 : 0);
}

hipError_t launch_debug_trace_clustered(const DevScene& sc, const float* rays, float* out, int64_t n, int32_t info[4],
                                        hipStream_t stream) {
    const int block = 256;
    const size_t lds = debug_clustered_lds_bytes(sc, block);
    // (the caller refuses a scene without clusters with a message of its own; the staged scene must fit a block)
    if (sc.nbrute <= 0 || sc.ncluster <= 0 || lds > 64 * 1024 || n > (int64_t)INT_MAX * block) return hipErrorInvalidValue;
    // what the kernel walks, as launch_pick notes it for a render launch (rt_debug_last_launch out[17..19])
    const int shell = sc.shell != 0;
    info[0] = sc.ncluster;
    info[1] = shell;
    info[2] = shell && sc.near_floor != 0.0f;
    info[3] = shell && (sc.host_flags & kHostQuad) != 0;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(debug_trace_clustered_kernel, dim3((unsigned)((n + block - 1) / block)), dim3(block), lds, stream,
                       sc, rays, out, n);
    return hipGetLastError();
}

size_t debug_fn_scratch_bytes(int fn, int64_t n) {
    // hemi: tri_shade (n float4) | frames (3 n float4) | two material rows
    return fn == RT_FN_HEMI ? (size_t)n * 4 * sizeof(float4) + 2 * kMatF * sizeof(float) : 0;
}

hipError_t launch_debug_fn(const DevScene& sc, int fn, const float* in, float* out, int64_t n, void* scratch,
                           hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 block(256), grid((unsigned)((n + 255) / 256));
    switch (fn) {
        case RT_FN_CAMERA: hipLaunchKernelGGL(debug_camera_kernel, grid, block, 0, stream, in, out, n); break;
        case RT_FN_SUN: hipLaunchKernelGGL(debug_sun_kernel, grid, block, 0, stream, in, out, n); break;
        case RT_FN_HEMI: {
            if (n > INT_MAX) return hipErrorInvalidValue;
            float4* shade = static_cast<float4*>(scratch);
            float4* frame = shade + n;
            float* mat = reinterpret_cast<float*>(frame + 3 * n);
            hipLaunchKernelGGL(debug_hemi_scene_kernel, grid, block, 0, stream, in, shade, mat, n);
            hipLaunchKernelGGL(prep_frames_kernel, grid, block, 0, stream, (const float4*)shade, (const float*)mat,
                               (int)n, frame);
            hipLaunchKernelGGL(debug_hemi_kernel, grid, block, 0, stream, in, (const float4*)shade,
                               (const float4*)frame, out, n);
            break;
        }
        case RT_FN_GGX: hipLaunchKernelGGL(debug_ggx_kernel, grid, block, 0, stream, in, out, n); break;
        case RT_FN_IBL:
            if (!sc.ibl_sum || sc.ibl_w <= 0 || sc.ibl_h <= 0) return hipErrorInvalidValue;
            hipLaunchKernelGGL(debug_ibl_kernel, grid, block, 0, stream, sc, in, out, n);
            break;
        case RT_FN_MT_REF: hipLaunchKernelGGL(debug_mt_kernel<false>, grid, block, 0, stream, in, out, n); break;
        case RT_FN_MT_FAST: hipLaunchKernelGGL(debug_mt_kernel<true>, grid, block, 0, stream, in, out, n); break;
        case RT_FN_BOX_REF: hipLaunchKernelGGL(debug_box_ref_kernel, grid, block, 0, stream, in, out, n); break;
        case RT_FN_BOX_FAST: hipLaunchKernelGGL(debug_box_fast_kernel, grid, block, 0, stream, in, out, n); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace rt
