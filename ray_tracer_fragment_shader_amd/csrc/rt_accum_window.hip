// rt_accum_window.hip — the depth-RT_ACCUM_WINDOW_B instances of the windowed accumulating render's kernel (rt_sampled.hpp).  The
// Makefile compiles this file once per bounce depth (rt_accum_window_b<B>.o), in parallel with the render kernels' units.
#include "rt_sampled.hpp"

#ifndef RT_ACCUM_WINDOW_B
#error "compile with -DRT_ACCUM_WINDOW_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_accum_window<RT_ACCUM_WINDOW_B>(const SampledLaunch& L) {
    return launch_accum_window_impl<RT_ACCUM_WINDOW_B>(L);
}
}  // namespace rtk
