// rt_motion.hip — the depth-RT_MOTION_B instances of the motion-blur kernel (rt_sampled.hpp).  The Makefile compiles this
// file once per bounce depth (rt_motion_b<B>.o), in parallel with the render kernels' translation units.
#include "rt_sampled.hpp"

#ifndef RT_MOTION_B
#error "compile with -DRT_MOTION_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_motion<RT_MOTION_B>(const SampledLaunch& L) { return launch_motion_impl<RT_MOTION_B>(L); }
}  // namespace rtk
