// rt_lens_adaptive.hip — the depth-RT_LENS_ADAPTIVE_B instances of the adaptive lens render's coarse and refine kernels
// (rt_sampled.hpp).  The Makefile compiles this file once per bounce depth (rt_lens_adaptive_b<B>.o), in parallel with
// the render kernels' translation units.
#include "rt_sampled.hpp"

#ifndef RT_LENS_ADAPTIVE_B
#error "compile with -DRT_LENS_ADAPTIVE_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_lens_coarse<RT_LENS_ADAPTIVE_B>(const SampledLaunch& L) {
    return launch_lens_coarse_impl<RT_LENS_ADAPTIVE_B>(L);
}
template <>
hipError_t launch_lens_refine<RT_LENS_ADAPTIVE_B>(const SampledLaunch& L) {
    return launch_lens_refine_impl<RT_LENS_ADAPTIVE_B>(L);
}
}  // namespace rtk
