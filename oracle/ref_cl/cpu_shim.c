/* cpu_shim.c -- TEST INFRASTRUCTURE ONLY.  Lets the reference's own kernel
 * text run on a CPU, with no OpenCL runtime.
 *
 * oracle/Makefile compiles oracle/ref_cl/kat.cl (which includes the reference's
 * Raytracing.cl where it lies) for the host with clang's OpenCL front end; every
 * __kernel becomes an ordinary C function and the OpenCL builtins it calls are
 * left as undefined symbols under their mangled names.  This file defines
 * exactly those symbols, from the numerics contract (csrc/rtm.h), plus the
 * driver that loops a kernel over its work-items.  It is compiled like the
 * oracle (-ffp-contract=off: contraction only where rtm.h says fmaf); the
 * reference keeps OpenCL's default contraction.  So a frame rendered through
 * this library is "the reference's program text under the contract", and the
 * oracle (oracle/rt_oracle.c) has to equal it bit for bit.
 *
 * Nothing of the reference is copied here.  Needs clang (ext_vector_type is
 * how the OpenCL vector types are passed); x86-64 System V only, as the recipe
 * fixes the target.
 */
#include <stddef.h>
#include <stdint.h>
#include <math.h>
#include "rtm.h"

typedef float cl_f3 __attribute__((ext_vector_type(3)));
typedef float cl_f4 __attribute__((ext_vector_type(4)));
typedef int cl_i2 __attribute__((ext_vector_type(2)));

#define CL_NAME(s) __asm__(s)

static inline rtm_f3 in3(cl_f3 v) { return rtm_v3(v.x, v.y, v.z); }
static inline cl_f3 out3(rtm_f3 v) { cl_f3 r; r.x = v.x; r.y = v.y; r.z = v.z; return r; }

/* ---- scalar builtins ---- */
float cl_sin(float x) CL_NAME("_Z3sinf");
float cl_cos(float x) CL_NAME("_Z3cosf");
float cl_tan(float x) CL_NAME("_Z3tanf");
float cl_asin(float x) CL_NAME("_Z4asinf");
float cl_acos(float x) CL_NAME("_Z4acosf");
float cl_atan2(float y, float x) CL_NAME("_Z5atan2ff");
float cl_sqrt(float x) CL_NAME("_Z4sqrtf");
float cl_fabs(float x) CL_NAME("_Z4fabsf");
float cl_fmax(float a, float b) CL_NAME("_Z4fmaxff");
float cl_fmin(float a, float b) CL_NAME("_Z4fminff");
float cl_pown(float x, int n) CL_NAME("_Z4pownfi");

float cl_sin(float x) { return rtm_sin(x); }
float cl_cos(float x) { return rtm_cos(x); }
float cl_tan(float x) { return rtm_tan(x); }
float cl_asin(float x) { return rtm_asin(x); }
float cl_acos(float x) { return rtm_acos(x); }
float cl_atan2(float y, float x) { return rtm_atan2(y, x); }
float cl_sqrt(float x) { return sqrtf(x); }
float cl_fabs(float x) { return rtm_fabs(x); }
float cl_fmax(float a, float b) { return rtm_fmax(a, b); }
float cl_fmin(float a, float b) { return rtm_fmin(a, b); }
/* The products the oracle spells for the two exponents the kernel uses; a plain
 * loop for the rest (only the reference's unused light-sampling code gets there). */
float cl_pown(float x, int n) {
    if (n == 2) return x * x;
    if (n == 5) return ((x * x) * (x * x)) * x;
    float r = 1.0f;
    for (int k = 0; k < (n < 0 ? -n : n); ++k) r = r * x;
    return n < 0 ? 1.0f / r : r;
}

/* ---- geometric builtins ---- */
float cl_dot(cl_f3 a, cl_f3 b) CL_NAME("_Z3dotDv3_fS_");
cl_f3 cl_cross(cl_f3 a, cl_f3 b) CL_NAME("_Z5crossDv3_fS_");
float cl_length(cl_f3 v) CL_NAME("_Z6lengthDv3_f");
cl_f3 cl_normalize(cl_f3 v) CL_NAME("_Z9normalizeDv3_f");
cl_f4 cl_normalize4(cl_f4 v) CL_NAME("_Z9normalizeDv4_f");

float cl_dot(cl_f3 a, cl_f3 b) { return rtm_dot(in3(a), in3(b)); }
cl_f3 cl_cross(cl_f3 a, cl_f3 b) { return out3(rtm_cross(in3(a), in3(b))); }
float cl_length(cl_f3 v) { return sqrtf(rtm_dot(in3(v), in3(v))); }
cl_f3 cl_normalize(cl_f3 v) { return out3(rtm_normalize(in3(v))); }
cl_f4 cl_normalize4(cl_f4 v) {
    const rtm_f4 r = rtm_normalize4(rtm_v4(v.x, v.y, v.z, v.w));
    cl_f4 o; o.x = r.x; o.y = r.y; o.z = r.z; o.w = r.w;
    return o;
}

/* ---- work-item id ---- */
static _Thread_local size_t g_gid;
size_t cl_get_global_id(unsigned dim) CL_NAME("_Z13get_global_idj");
size_t cl_get_global_id(unsigned dim) { return dim == 0 ? g_gid : 0; }

/* ---- the image: what the kernel holds as image2d_t points at one of these ----
 * read_imagef through the reference's sampler (unnormalised, clamp to edge,
 * linear) at integer coordinates is the project's definition (SURVEY.md
 * Appendix A.8): the sum of the four clamped texels (x-1..x, y-1..y) times
 * 1/1020.  The same definition as ibl_fetch of the oracle, so this library
 * does not pin the image fetch; it pins everything around it. */
typedef struct { int32_t w, h; const uint8_t* rgba; } ref_image;

int cl_image_width(const ref_image* im) CL_NAME("_Z15get_image_width14ocl_image2d_ro");
int cl_image_height(const ref_image* im) CL_NAME("_Z16get_image_height14ocl_image2d_ro");
cl_f4 cl_read_imagef(const ref_image* im, const void* sampler, cl_i2 xy)
    CL_NAME("_Z11read_imagef14ocl_image2d_ro11ocl_samplerDv2_i");
void* __translate_sampler_initializer(int v);

int cl_image_width(const ref_image* im) { return im->w; }
int cl_image_height(const ref_image* im) { return im->h; }
void* __translate_sampler_initializer(int v) { (void)v; return NULL; }

static inline int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

cl_f4 cl_read_imagef(const ref_image* im, const void* sampler, cl_i2 xy) {
    (void)sampler;
    const int W = im->w, H = im->h, x = xy.x, y = xy.y;
    const int x0 = clampi(x > -2147483647 ? x - 1 : x, W - 1), x1 = clampi(x, W - 1);
    const int y0 = clampi(y > -2147483647 ? y - 1 : y, H - 1), y1 = clampi(y, H - 1);
    const uint8_t* t00 = im->rgba + 4 * ((int64_t)y0 * W + x0);
    const uint8_t* t10 = im->rgba + 4 * ((int64_t)y0 * W + x1);
    const uint8_t* t01 = im->rgba + 4 * ((int64_t)y1 * W + x0);
    const uint8_t* t11 = im->rgba + 4 * ((int64_t)y1 * W + x1);
    float c[4];
    for (int k = 0; k < 4; ++k) {
        const float s = (float)((int)t00[k] + (int)t10[k] + (int)t01[k] + (int)t11[k]);
        c[k] = s * (1.0f / 1020.0f);
    }
    cl_f4 o; o.x = c[0]; o.y = c[1]; o.z = c[2]; o.w = c[3];
    return o;
}

/* ---- driver ----
 * Every kernel argument is a pointer or a 32-bit integer, i.e. one INTEGER-class
 * eightbyte each in the x86-64 System V convention, in registers and on the
 * stack alike, and surplus arguments are the caller's to clean up.  So one call
 * shape serves every kernel: its arguments widened to 64 bits, padded to
 * REF_MAX_ARGS. */
#define REF_MAX_ARGS 16
typedef uint64_t A;
typedef void (*ref_kernel)(A, A, A, A, A, A, A, A, A, A, A, A, A, A, A, A);

int ref_max_args(void) { return REF_MAX_ARGS; }

/* Runs work-items 0 .. n-1 of `kernel`.  Returns 0, or -1 on bad arguments. */
int ref_run(void (*kernel)(void), const uint64_t* args, int nargs, int64_t n, int nthreads) {
    if (!kernel || nargs < 0 || nargs > REF_MAX_ARGS || n < 0) return -1;
    A a[REF_MAX_ARGS] = {0};
    for (int k = 0; k < nargs; ++k) a[k] = args[k];
    const ref_kernel fn = (ref_kernel)kernel;
    if (nthreads <= 0) nthreads = 1;
#if defined(_OPENMP)
#pragma omp parallel for schedule(dynamic, 64) num_threads(nthreads)
#endif
    for (int64_t t = 0; t < n; ++t) {
        g_gid = (size_t)t;
        fn(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15]);
    }
    return 0;
}
