// Temporal reprojection (rt_reproject_device, rt_accum_reproject; include/rt_api.h): the previous view's frame and
// guides gathered into the current view and blended by sample counts.  One image-space kernel in a translation
// unit of its own -- no other code object changes, and nothing is shared with rt_denoise.hip through a header
// (doing so reorders guides_kernel).  No ray, no LDS, no atomics, no scratch.
//
// Numerics: the operation is defined step by step in rt_api.h and uses only IEEE + - * /, floor, min, max, abs and
// compares in that order (this file is compiled with -ffp-contract=off like every other): a float32 restatement in
// numpy is its exact oracle (tests/reproject_ref.py).
#include <algorithm>

#include "rt_internal.h"
#include "rtm.h"

namespace rt {

namespace {
constexpr int kRpBlock = 256;
constexpr int kRpMaxBlocks = 4096;   // grid-stride above this: 16 blocks per CU

// G1 = P | f and G2 = a | m of a guide (rt_api.h): the int words
__device__ __forceinline__ int word(float x) { return __float_as_int(x); }

// One lane per current pixel.  The basis and the parameters are kernel arguments: wave-uniform, in SGPRs.
// A pixel without history -- step 0 and every "no history" exit of the definition -- falls through to the one
// store site with its inputs' own words: 15 floats copied.
__global__ void __launch_bounds__(kRpBlock) reproject_kernel(const float* __restrict__ prev_rgb,
                                                             const float4* __restrict__ prev_g,
                                                             const float* __restrict__ cur_rgb,
                                                             const float4* __restrict__ cur_g, int64_t npix, int W,
                                                             float Wf, float Hf, ReprojectBasis B,
                                                             ReprojectParams P, float* __restrict__ out_rgb,
                                                             float4* __restrict__ out_g) {
    for (int64_t p = (int64_t)blockIdx.x * kRpBlock + threadIdx.x; p < npix; p += (int64_t)gridDim.x * kRpBlock) {
        const float4 g0 = cur_g[3 * p], g1 = cur_g[3 * p + 1], g2 = cur_g[3 * p + 2];
        float r = cur_rgb[3 * p], g = cur_rgb[3 * p + 1], b = cur_rgb[3 * p + 2];
        float fw = g1.w;
        const int fp = word(g1.w);
        if (fp > 0) {
            // 1. the pixel's first hit in the previous camera's frame
            const float vx = g1.x - B.pos[0], vy = g1.y - B.pos[1], vz = g1.z - B.pos[2];
            const float lx = (B.m[0] * vx + B.m[1] * vy) + B.m[2] * vz;
            const float ly = (B.m[3] * vx + B.m[4] * vy) + B.m[5] * vz;
            const float lz = (B.m[6] * vx + B.m[7] * vy) + B.m[8] * vz;
            if (ly > 0.0f) {
                // 2. its continuous pixel coordinates there
                const float t = B.f / ly;
                const float u = (lx * t + 0.5f) * B.cam6;
                const float vv = (0.5f - lz * t) * B.cam6;
                if (u >= -1.0f && u < Wf && vv >= -1.0f && vv < Hf) {
                    const float c0 = floorf(u), r0 = floorf(vv);
                    const float fu = u - c0, fv = vv - r0;
                    const int ci = (int)c0, ri = (int)r0;
                    // 3. the four taps; their G1 words are loaded together, from pixel 0 where a tap leaves the frame
                    int64_t q[4];
                    bool in[4];
                    float4 q1[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int c = ci + (k & 1), rr = ri + (k >> 1);
                        q[k] = ((int64_t)rr + 1) * W + c - 1;
                        in[k] = c >= 0 && c < W && rr >= 0 && q[k] < npix;
                        q1[k] = prev_g[3 * (in[k] ? q[k] : 0) + 1];
                    }
                    const int mp = word(g2.w);
                    const float spk = P.sigma_p * g0.w;
                    float ax = 0.0f, ay = 0.0f, az = 0.0f, ws = 0.0f, hs = 0.0f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int fq = word(q1[k].w);
                        if (!in[k] || fq <= 0) continue;
                        const float4 q2 = prev_g[3 * q[k] + 2];
                        if (word(q2.w) != mp) continue;
                        const float4 q0 = prev_g[3 * q[k]];
                        if (!((g0.x * q0.x + g0.y * q0.y) + g0.z * q0.z >= P.normal_min)) continue;
                        const float dx = q1[k].x - g1.x, dy = q1[k].y - g1.y, dz = q1[k].z - g1.z;
                        if (!(rtm_fabs((g0.x * dx + g0.y * dy) + g0.z * dz) <= spk)) continue;
                        const float bw = ((k & 1) ? fu : 1.0f - fu) * ((k >> 1) ? fv : 1.0f - fv);
                        const float* pc = prev_rgb + 3 * q[k];
                        ax = ax + bw * (pc[0] / q2.x);
                        ay = ay + bw * (pc[1] / q2.y);
                        az = az + bw * (pc[2] / q2.z);
                        ws = ws + bw;
                        hs = hs + bw * (float)fq;
                    }
                    // 4., 5. the history's colour and length, blended with the pixel's own by sample counts
                    if (ws >= P.min_weight && ws > 0.0f) {
                        const float hq = hs / ws;
                        const float h = hq < P.max_history ? hq : P.max_history;
                        const float s = (float)fp, tot = h + s;
                        const float xr = ((ax / ws) * h + (r / g2.x) * s) / tot;
                        const float xg = ((ay / ws) * h + (g / g2.y) * s) / tot;
                        const float xb = ((az / ws) * h + (b / g2.z) * s) / tot;
                        r = rtm_fmax(rtm_fmin(xr * g2.x, 1.0f), 0.0f);
                        g = rtm_fmax(rtm_fmin(xg * g2.y, 1.0f), 0.0f);
                        b = rtm_fmax(rtm_fmin(xb * g2.z, 1.0f), 0.0f);
                        fw = __int_as_float(tot < 2147483648.0f ? (int)tot : 2147483647);
                    }
                }
            }
        }
        out_rgb[3 * p] = r;
        out_rgb[3 * p + 1] = g;
        out_rgb[3 * p + 2] = b;
        out_g[3 * p] = g0;
        out_g[3 * p + 1] = make_float4(g1.x, g1.y, g1.z, fw);
        out_g[3 * p + 2] = g2;
    }
}
}  // namespace

hipError_t launch_reproject(const float* d_prev_rgb, const float4* d_prev_guides, const float* d_cur_rgb,
                            const float4* d_cur_guides, int64_t npix, int width, const ReprojectBasis& basis,
                            const ReprojectParams& params, float* d_out_rgb, float4* d_out_guides,
                            hipStream_t stream) {
    if (npix <= 0) return hipSuccess;
    if (!d_prev_rgb || !d_prev_guides || !d_cur_rgb || !d_cur_guides || !d_out_rgb || !d_out_guides || width < 1)
        return hipErrorInvalidValue;
    const int64_t H = (npix + width - 1) / width;
    const int64_t blocks = std::min<int64_t>((npix + kRpBlock - 1) / kRpBlock, kRpMaxBlocks);
    hipLaunchKernelGGL(reproject_kernel, dim3((unsigned)blocks), dim3(kRpBlock), 0, stream, d_prev_rgb, d_prev_guides,
                       d_cur_rgb, d_cur_guides, npix, width, (float)width, (float)H, basis, params, d_out_rgb,
                       d_out_guides);
    return hipGetLastError();
}

}  // namespace rt
