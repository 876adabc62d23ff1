// rt_adaptive.hip — the depth-RT_ADAPTIVE_B instances of the refine kernel (rt_sampled.hpp).  The Makefile compiles
// this file once per bounce depth (rt_adaptive_b<B>.o), in parallel with the render kernels' translation units.
#include "rt_sampled.hpp"

#ifndef RT_ADAPTIVE_B
#error "compile with -DRT_ADAPTIVE_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_refine<RT_ADAPTIVE_B>(const SampledLaunch& L) { return launch_refine_impl<RT_ADAPTIVE_B>(L); }
}  // namespace rtk
