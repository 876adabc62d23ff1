// rt_soft.hip — the depth-RT_SOFT_B instances of the soft-shadow kernel (rt_sampled.hpp).  The Makefile compiles this
// file once per bounce depth (rt_soft_b<B>.o), in parallel with the render kernels' translation units.
#include "rt_sampled.hpp"

#ifndef RT_SOFT_B
#error "compile with -DRT_SOFT_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_soft<RT_SOFT_B>(const SampledLaunch& L) { return launch_soft_impl<RT_SOFT_B>(L); }
}  // namespace rtk
