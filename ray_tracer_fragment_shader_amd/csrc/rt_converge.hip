// rt_converge.hip — the depth-RT_CONVERGE_B instances of the converging render's kernel (rt_sampled.hpp).  The Makefile
// compiles this file once per bounce depth (rt_converge_b<B>.o), in parallel with the render kernels' translation units.
#include "rt_sampled.hpp"

#ifndef RT_CONVERGE_B
#error "compile with -DRT_CONVERGE_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_converge<RT_CONVERGE_B>(const SampledLaunch& L) {
    return launch_converge_impl<RT_CONVERGE_B>(L);
}
}  // namespace rtk
