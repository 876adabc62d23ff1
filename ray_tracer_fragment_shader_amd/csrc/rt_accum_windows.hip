// rt_accum_windows.hip — the depth-RT_ACCUM_WINDOWS_B instances of the accumulating render's list kernel (rt_sampled.hpp).  The
// Makefile compiles this file once per bounce depth (rt_accum_windows_b<B>.o), in parallel with the render kernels' units.
#include "rt_sampled.hpp"

#ifndef RT_ACCUM_WINDOWS_B
#error "compile with -DRT_ACCUM_WINDOWS_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_accum_windows<RT_ACCUM_WINDOWS_B>(const SampledLaunch& L) {
    return launch_accum_windows_impl<RT_ACCUM_WINDOWS_B>(L);
}
}  // namespace rtk
