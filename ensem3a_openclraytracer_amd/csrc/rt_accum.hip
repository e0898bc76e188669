// The kernels of a progressive accumulation's add (rt_accum_*): the ACC instantiations of render_kernel and
// render_resume_kernel and their launcher, launch_accum, compiled from rt_kernels.hip in a translation
// unit of their own so that the one-shot kernels' code object is untouched by them.
#define RT_ACCUM_TU 1
#include "rt_kernels.hip"
