// rt_jitter.hip — the depth-RT_JITTER_B instances of the jittered render's kernel (rt_sampled.hpp).  The Makefile
// compiles this file once per bounce depth (rt_jitter_b<B>.o), in parallel with the render kernels' translation units.
#include "rt_sampled.hpp"

#ifndef RT_JITTER_B
#error "compile with -DRT_JITTER_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_jitter<RT_JITTER_B>(const SampledLaunch& L) {
    return launch_jitter_impl<RT_JITTER_B>(L);
}
}  // namespace rtk
