// rt_accum.hip — the depth-RT_ACCUM_B instances of the accumulating render's kernel (rt_sampled.hpp).  The Makefile
// compiles this file once per bounce depth (rt_accum_b<B>.o), in parallel with the render kernels' translation units.
#include "rt_sampled.hpp"

#ifndef RT_ACCUM_B
#error "compile with -DRT_ACCUM_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_accum<RT_ACCUM_B>(const SampledLaunch& L) {
    return launch_accum_impl<RT_ACCUM_B>(L);
}
}  // namespace rtk
