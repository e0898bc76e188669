// The kernels of adaptive sampling (rt_accum_mark, rt_accum_select*, rt_accum_add_selected): the listed
// instantiations of render_kernel and render_resume_kernel (ACC = kAccListed) with their launcher,
// launch_accum_listed, and the mark, select and compaction kernels, compiled from rt_kernels.hip in a
// translation unit of their own so that the code objects of the one-shot kernels and of the adds
// (rt_accum.hip) are untouched by them.
#define RT_ACCUM_TU 2
#include "rt_kernels.hip"
