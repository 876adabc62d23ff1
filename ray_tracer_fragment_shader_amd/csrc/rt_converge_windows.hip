// rt_converge_windows.hip — the depth-RT_CONVERGE_WINDOWS_B instances of the converging render's list kernel (rt_sampled.hpp).  The
// Makefile compiles this file once per bounce depth (rt_converge_windows_b<B>.o), in parallel with the render kernels' units.
#include "rt_sampled.hpp"

#ifndef RT_CONVERGE_WINDOWS_B
#error "compile with -DRT_CONVERGE_WINDOWS_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_converge_windows<RT_CONVERGE_WINDOWS_B>(const SampledLaunch& L) {
    return launch_converge_windows_impl<RT_CONVERGE_WINDOWS_B>(L);
}
}  // namespace rtk
