// rt_shutter.hip — the depth-RT_SHUTTER_B instances of the shutter render's kernel (rt_sampled.hpp).  The Makefile
// compiles this file once per bounce depth (rt_shutter_b<B>.o), in parallel with the render kernels' translation units.
#include "rt_sampled.hpp"

#ifndef RT_SHUTTER_B
#error "compile with -DRT_SHUTTER_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_shutter<RT_SHUTTER_B>(const SampledLaunch& L) {
    return launch_shutter_impl<RT_SHUTTER_B>(L);
}
}  // namespace rtk
