// Denoised previews (rt_accum_guides*, rt_denoise_device, rt_accum_denoise; include/rt_api.h): the first-hit
// guide buffers out of an accumulation's state, and the edge-aware a-trous filter they drive.  A translation
// unit of its own -- no render kernel's code object changes -- that takes the camera ray (LaunchConst,
// camera_dir) from rt_device.h, so a guide's position is built from the direction the render kernels trace.
//
// Numerics: the filter is defined operation by operation in rt_api.h and uses only IEEE + - * /, max, min and
// abs in that order (this file is compiled with -ffp-contract=off like every other): a float32 restatement in
// numpy is its exact oracle (tests/denoise_ref.py).
#include "rt_device.h"

namespace rt {

namespace {
constexpr int kDnBlock = 256;   // 4 waves; in the filter passes each wave is one 64-pixel row segment

__device__ __forceinline__ bool dn_tile_pixel(int64_t p, int W, int row0, int row_step, int64_t npix, int* i) {
    const int64_t krow = p / W;
    const int64_t i64 = ((int64_t)row0 + krow * row_step) * W + (p - krow * W);
    *i = (int)i64;
    return i64 < npix;   // (npix < 2^31: check_frame)
}

// rt_accum_guides: G0 = n | k, G1 = P | f, G2 = a | m of every tile pixel (rt_api.h)
__global__ void __launch_bounds__(kDnBlock) guides_kernel(const float4* __restrict__ state,
                                                          const float4* __restrict__ tri_shade,
                                                          const float* __restrict__ mat, int ntri, int nmat, int64_t n,
                                                          int W, int row0, int row_step, int64_t npix,
                                                          const LaunchConst* __restrict__ lconst,
                                                          float4* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= n) return;
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    float4 g1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0));
    float4 g2 = make_float4(1.0f, 1.0f, 1.0f, __int_as_float(-1));
    int i;
    if (dn_tile_pixel(p, W, row0, row_step, npix, &i)) {
        const float4 a = state[2 * p], b = state[2 * p + 1];
        const int tc = __float_as_int(b.z), s = __float_as_int(b.w);
        if (tc >= 0 && tc < ntri) {
            const LaunchConst& C = *lconst;
            const float4 sh = tri_shade[tc];
            const int m = __float_as_int(sh.w);
            const float kc = a.w;
            const rtm_f3 d = camera_dir(C, W, i);
            g0 = make_float4(sh.x, sh.y, sh.z, kc);
            g1.x = C.position.x + d.x * kc;
            g1.y = C.position.y + d.y * kc;
            g1.z = C.position.z + d.z * kc;
            g2.w = __int_as_float(m);
            if (m >= 0 && m < nmat) {
                const int type = (int)mat[kMatF * m];
                if (type == 1 || type == 2) {
                    g1.w = __int_as_float(s);
                    g2.x = rtm_fmax(mat[kMatF * m + 1], 0.01f);
                    g2.y = rtm_fmax(mat[kMatF * m + 2], 0.01f);
                    g2.z = rtm_fmax(mat[kMatF * m + 3], 0.01f);
                }
            }
        }
    }
    out[3 * p + 0] = g0;
    out[3 * p + 1] = g1;
    out[3 * p + 2] = g2;
}

// The filter's layout: X = x.rgb | f (ping-pongs), N = n | k, Pp = P (constant over the passes), one float4 per
// frame pixel each, so that a tap is one contiguous 16-byte load per lane.  x = c / a where the pixel is
// filterable (f > 0); elsewhere x = c and f = 0, which is all a tap asks of such a pixel.
__global__ void __launch_bounds__(kDnBlock) denoise_pack_kernel(const float* __restrict__ rgb,
                                                                const float4* __restrict__ guides, int64_t npix,
                                                                float4* __restrict__ X, float4* __restrict__ N,
                                                                float4* __restrict__ Pp) {
    const int64_t p = (int64_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (p >= npix) return;
    const float4 g0 = guides[3 * p], g1 = guides[3 * p + 1], g2 = guides[3 * p + 2];
    const int f = __float_as_int(g1.w);
    float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
    if (f > 0) {
        r = r / g2.x;
        g = g / g2.y;
        b = b / g2.z;
    }
    X[p] = make_float4(r, g, b, __int_as_float(f > 0 ? f : 0));
    N[p] = g0;
    Pp[p] = g1;
}

// The weight of a tap on a filterable pixel q of filterable p (rt_api.h, "Pass i"): w = (h (wn wp)) wc, every
// operation in the order written there.  spk = sigma_p k_p and sc2 are p's own, computed once per pass.
__device__ __forceinline__ float tap_weight(float4 np, float4 pp, float4 xp, float4 nq, float4 pq, float4 xq, float h,
                                            int nsq, float spk, float sc2) {
    const float t = rtm_fmax(0.0f, (np.x * nq.x + np.y * nq.y) + np.z * nq.z);
    float wn = t;
    for (int k = 0; k < nsq; ++k) wn = wn * wn;
    const float ddx = pq.x - pp.x, ddy = pq.y - pp.y, ddz = pq.z - pp.z;
    const float dpl = rtm_fabs((np.x * ddx + np.y * ddy) + np.z * ddz);
    const float a_ = dpl / spk;
    const float wp = 1.0f / (1.0f + a_ * a_);
    const float cr = xq.x - xp.x, cg = xq.y - xp.y, cb = xq.z - xp.z;
    const float d2 = (cr * cr + cg * cg) + cb * cb;
    const float wc = 1.0f / (1.0f + d2 / sc2);
    return (h * (wn * wp)) * wc;
}

__device__ __forceinline__ float tap_k(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// what a pass writes for pixel p: a pixel that is not filterable passes through (the last pass copies the
// input's own words), a filtered one is stored for the next pass or, by the last pass, remodulated and clamped
template <bool LAST>
__device__ __forceinline__ void pass_through(int64_t p, float4 xp, const float* __restrict__ rgb,
                                             float4* __restrict__ Xout, float* __restrict__ out) {
    if (LAST) {
        const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
        out[3 * p] = r;
        out[3 * p + 1] = g;
        out[3 * p + 2] = b;
    } else {
        Xout[p] = xp;
    }
}
template <bool LAST>
__device__ __forceinline__ void pass_store(int64_t p, float rx, float ry, float rz, float f,
                                           const float4* __restrict__ guides, float4* __restrict__ Xout,
                                           float* __restrict__ out) {
    if (LAST) {
        const float4 a = guides[3 * p + 2];
        out[3 * p] = rtm_fmax(rtm_fmin(rx * a.x, 1.0f), 0.0f);
        out[3 * p + 1] = rtm_fmax(rtm_fmin(ry * a.y, 1.0f), 0.0f);
        out[3 * p + 2] = rtm_fmax(rtm_fmin(rz * a.z, 1.0f), 0.0f);
    } else {
        Xout[p] = make_float4(rx, ry, rz, f);
    }
}

// One pass of the filter at `step` (rt_api.h, "Pass i"), taps straight from global memory.  LAST: the pass
// remodulates and writes the frame -- clamp(x' * a) where the pixel is filterable, the input's own words elsewhere.
template <bool LAST>
__global__ void __launch_bounds__(kDnBlock) denoise_pass_kernel(const float4* __restrict__ Xin,
                                                                const float4* __restrict__ N,
                                                                const float4* __restrict__ Pp,
                                                                float4* __restrict__ Xout, const float* __restrict__ rgb,
                                                                const float4* __restrict__ guides,
                                                                float* __restrict__ out, int64_t npix, int W, int64_t H,
                                                                int64_t segs_per_row, int64_t nsegs, int step, int nsq,
                                                                float sigma_c, float sigma_p) {
    const int64_t seg = (int64_t)blockIdx.x * (kDnBlock / 64) + (threadIdx.x >> 6);
    if (seg >= nsegs) return;
    const int64_t y = seg / segs_per_row;
    const int64_t x = (seg - y * segs_per_row) * 64 + (threadIdx.x & 63);
    if (x >= W) return;
    const int64_t p = y * W + x;
    if (p >= npix) return;
    const float4 xp = Xin[p];
    const int sp = __float_as_int(xp.w);
    if (sp <= 0) {
        pass_through<LAST>(p, xp, rgb, Xout, out);
        return;
    }
    const float4 np = N[p], pp = Pp[p];
    const float sc2 = ((sigma_c * sigma_c) / (float)sp) / (float)(step * step);
    const float spk = sigma_p * np.w;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int64_t qy = y + (int64_t)dy * step;   // (the wave's row: uniform)
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float h = tap_k(dx) * tap_k(dy);
            float w;
            float4 xq;
            if (dx == 0 && dy == 0) {
                w = h;
                xq = xp;
            } else {
                const int64_t qx = x + (int64_t)dx * step;
                if (qx < 0 || qx >= W) continue;
                const int64_t q = qy * W + qx;
                if (q >= npix) continue;
                xq = Xin[q];
                if (__float_as_int(xq.w) <= 0) continue;
                w = tap_weight(np, pp, xp, N[q], Pp[q], xq, h, nsq, spk, sc2);
            }
            ax = ax + w * xq.x;
            ay = ay + w * xq.y;
            az = az + w * xq.z;
            ws = ws + w;
        }
    }
    pass_store<LAST>(p, ax / ws, ay / ws, az / ws, xp.w, guides, Xout, out);
}

// The pass at step 1 with the block's tile -- 4 rows of 64 pixels -- and its halo of 2 pixels staged in LDS
// (X, N and P: 26 KB), each tap one ds_read_b128 per lane.  It is the one step at which staging beats the
// taps from global memory (at step 2 the halo makes the tile 41 KB and the pass slower).  A staged pixel that lies
// outside the frame, past npix, or is not filterable is staged with f = 0, which is what gives its tap no weight.
// A wave reads 64 consecutive float4 of one staged row at a time, so the row pitch needs no padding against
// bank conflicts.  The taps, their order and every operation are the baseline's: the same bits.
template <bool LAST>
__global__ void __launch_bounds__(kDnBlock) denoise_pass_lds_kernel(const float4* __restrict__ Xin,
                                                                    const float4* __restrict__ N,
                                                                    const float4* __restrict__ Pp,
                                                                    float4* __restrict__ Xout,
                                                                    const float* __restrict__ rgb,
                                                                    const float4* __restrict__ guides,
                                                                    float* __restrict__ out, int64_t npix, int W,
                                                                    int64_t H, int64_t segs_per_row, int nsq,
                                                                    float sigma_c, float sigma_p) {
    constexpr int STEP = 1, HL = 2 * STEP, TW = 64 + 2 * HL, TH = kDnBlock / 64 + 2 * HL;
    __shared__ float4 sX[TH * TW], sN[TH * TW], sP[TH * TW];
    const int64_t by = (int64_t)blockIdx.x / segs_per_row;
    const int64_t bx = (int64_t)blockIdx.x - by * segs_per_row;
    const int64_t x0 = bx * 64 - HL, y0 = by * (kDnBlock / 64) - HL;
    for (int e = threadIdx.x; e < TH * TW; e += kDnBlock) {
        const int ly = e / TW, lx = e - ly * TW;
        const int64_t gy = y0 + ly, gx = x0 + lx;
        float4 xv = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0)), nv = xv, pv = xv;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int64_t q = gy * W + gx;
            if (q < npix) {
                xv = Xin[q];
                if (__float_as_int(xv.w) > 0) {
                    nv = N[q];
                    pv = Pp[q];
                }
            }
        }
        sX[e] = xv;
        sN[e] = nv;
        sP[e] = pv;
    }
    __syncthreads();
    const int ly = HL + (int)(threadIdx.x >> 6), lx = HL + (int)(threadIdx.x & 63);
    const int64_t y = y0 + ly, x = x0 + lx;
    if (x >= W || y >= H) return;
    const int64_t p = y * W + x;
    if (p >= npix) return;
    const int c = ly * TW + lx;
    const float4 xp = sX[c];
    const int sp = __float_as_int(xp.w);
    if (sp <= 0) {
        pass_through<LAST>(p, xp, rgb, Xout, out);
        return;
    }
    const float4 np = sN[c], pp = sP[c];
    const float sc2 = ((sigma_c * sigma_c) / (float)sp) / (float)(STEP * STEP);
    const float spk = sigma_p * np.w;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float h = tap_k(dx) * tap_k(dy);
            float w;
            float4 xq;
            if (dx == 0 && dy == 0) {
                w = h;
                xq = xp;
            } else {
                const int q = c + dy * STEP * TW + dx * STEP;
                xq = sX[q];
                if (__float_as_int(xq.w) <= 0) continue;
                w = tap_weight(np, pp, xp, sN[q], sP[q], xq, h, nsq, spk, sc2);
            }
            ax = ax + w * xq.x;
            ay = ay + w * xq.y;
            az = az + w * xq.z;
            ws = ws + w;
        }
    }
    pass_store<LAST>(p, ax / ws, ay / ws, az / ws, xp.w, guides, Xout, out);
}

inline unsigned dn_grid(int64_t n) { return (unsigned)((n + kDnBlock - 1) / kDnBlock); }
}  // namespace

size_t launch_const_bytes() { return sizeof(LaunchConst); }

hipError_t launch_accum_guides(const DevScene& sc, const FrameParams& fp, const float4* state, void* lconst,
                               float4* d_guides, hipStream_t stream) {
    if (fp.nloc <= 0) return hipSuccess;
    if (!state || !lconst || !d_guides) return hipErrorInvalidValue;
    LaunchConst* lc = static_cast<LaunchConst*>(lconst);
    hipLaunchKernelGGL(make_const_kernel, dim3(1), dim3(64), 0, stream, fp, lc);
    hipLaunchKernelGGL(guides_kernel, dim3(dn_grid(fp.nloc)), dim3(kDnBlock), 0, stream, state, sc.tri_shade, sc.mat,
                       sc.ntri, sc.nmat, fp.nloc, fp.width, fp.row0, fp.row_step, fp.npix, (const LaunchConst*)lc,
                       d_guides);
    return hipGetLastError();
}

size_t denoise_scratch_bytes(int64_t npix) { return (size_t)npix * 4 * sizeof(float4); }

hipError_t launch_denoise(const float* d_rgb, const float4* d_guides, int64_t npix, int width, int passes, int nsq,
                          float sigma_c, float sigma_p, bool lds, float4* scratch, float* d_out,
                          hipStream_t stream) {
    if (npix <= 0) return hipSuccess;
    if (!d_rgb || !d_guides || !scratch || !d_out || width < 1 || passes < 1) return hipErrorInvalidValue;
    float4* X[2] = {scratch, scratch + npix};
    const float4* N = scratch + 2 * npix;
    const float4* Pp = scratch + 3 * npix;
    const int64_t H = (npix + width - 1) / width;
    const int64_t segs_per_row = ((int64_t)width + 63) / 64;
    const int64_t nsegs = segs_per_row * H;
    constexpr int kRows = kDnBlock / 64;
    const int64_t blocks = (nsegs + kRows - 1) / kRows;          // baseline: 4 consecutive row segments
    const int64_t tiles = segs_per_row * ((H + kRows - 1) / kRows);   // LDS variant: 64 x 4 tiles
    if (blocks > 0x7fffffff || tiles > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(denoise_pack_kernel, dim3(dn_grid(npix)), dim3(kDnBlock), 0, stream, d_rgb, d_guides, npix, X[0],
                       scratch + 2 * npix, scratch + 3 * npix);
    for (int i = 0; i < passes; ++i) {
        const float4* in = X[i & 1];
        float4* o = X[(i + 1) & 1];
        const bool last = i + 1 == passes;
        const dim3 b(kDnBlock), gt((unsigned)tiles);
        if (i == 0 && lds) {
            if (last)
                hipLaunchKernelGGL(denoise_pass_lds_kernel<true>, gt, b, 0, stream, in, N, Pp, o, d_rgb, d_guides, d_out,
                                   npix, width, H, segs_per_row, nsq, sigma_c, sigma_p);
            else
                hipLaunchKernelGGL(denoise_pass_lds_kernel<false>, gt, b, 0, stream, in, N, Pp, o, d_rgb, d_guides, d_out,
                                   npix, width, H, segs_per_row, nsq, sigma_c, sigma_p);
        } else if (last) {
            hipLaunchKernelGGL(denoise_pass_kernel<true>, dim3((unsigned)blocks), b, 0, stream, in, N, Pp, o, d_rgb,
                               d_guides, d_out, npix, width, H, segs_per_row, nsegs, 1 << i, nsq, sigma_c, sigma_p);
        } else {
            hipLaunchKernelGGL(denoise_pass_kernel<false>, dim3((unsigned)blocks), b, 0, stream, in, N, Pp, o, d_rgb,
                               d_guides, d_out, npix, width, H, segs_per_row, nsegs, 1 << i, nsq, sigma_c, sigma_p);
        }
    }
    return hipGetLastError();
}

}  // namespace rt
